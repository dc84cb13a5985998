"""Guards of the planted-match list (tests/planted_cases.py) that need no GPU: what tests/test_gpu_planted.py compares the kernels
with is a valid stream of the case's input, no case hides behind a stored block, the list is what it was, the planted copies are
found -- and the oracle's own parse of them is the compiled reference's where that was built.

Shares of the cases with L >= 9 whose stream is shorter than the unplanted background's (geometry A; the condition is 0.60), as
measured with this generator (the background: 55,272 bytes at level 1 -- no match at all --, 34,089 at levels 2..6):

    mode                 pos     len     dist
    level 1 cold         0.869   0.917   0.788
    levels 2, 3 cold     0.881   0.925   0.721
    level 4              0.911   0.966   0.888
    level 5              0.912   0.966   0.948
    level 6              0.911   0.966   0.948
    level 1 warm 258     0.869   0.921   0.822
    level 1 warm 32768   1.000   1.000   0.944
    level 2 warm 4096    0.916   0.936   0.788
    level 3 warm 32768   0.916   0.936   0.885

(A copy that is not found is one the parse is not allowed to see: its
source lies in front of a cold packet, further back than the window, or the copy sits behind target = n - 258.)"""
import collections
import hashlib
import zlib

import pytest

import planted_cases as pc

WBITS = {0: 15, 1: 31, 2: -15}
HEADER = {0: 2, 1: 10, 2: 0}
TRAILER = {0: 4, 1: 8, 2: 0}
BITE = 0.60
COUNTS_A = {"pos": 2658, "len": 338, "dist": 269, "start": 772, "lazy": 282, "backcap": 24}
COUNTS_B = {4096: {"pos": 4350, "dist": 315, "start-far": 30}, 1000: {"pos": 4350, "dist": 228, "start-far": 30},
            777: {"pos": 4350, "dist": 225, "start-far": 30}}


def mode_id(m):
    return f"level{m[0]}" + (f"-warm{m[1]}" if m[1] else "")


@pytest.fixture(scope="module", params=pc.MODES, ids=mode_id)
def survey(request, oracle):
    """every case of every geometry once through the oracle in this mode: (mode, [(geometry, case, stream length, first block's
    type, inflates to the input)] -- the length without the container --, {geometry: the background's stream length})"""
    lvl, warm = request.param
    rows, base = [], {}
    for geometry, cases in [("A", pc.cases_a())] + [(P, pc.cases_b(P)) for P in pc.B_PACKETS]:
        P, n = pc.size_of(geometry)
        base[geometry] = len(oracle.encode_packets(pc.BACKGROUND[:n], 2, lvl, P, warm))
        for i, c in enumerate(cases):
            d, fmt = pc.plant(c, n), i % 3
            s = oracle.encode_packets(d, fmt, lvl, P, warm)
            try:
                ok = zlib.decompressobj(WBITS[fmt]).decompress(s) == d
            except zlib.error:
                ok = False
            rows.append((geometry, c, len(s) - HEADER[fmt] - TRAILER[fmt], (s[HEADER[fmt]] >> 1) & 3, ok))
    return request.param, rows, base


def test_oracle_streams_inflate_to_the_input(survey):
    mode, rows, _ = survey
    assert [(g, c) for g, c, _, _, ok in rows if not ok] == [], mode


def test_no_first_block_is_stored(survey):
    mode, rows, _ = survey
    assert [(g, c) for g, c, _, btype, _ in rows if btype == 0] == [], mode


def test_the_cases_bite(survey):
    """see the module's docstring: a condition on the list, not a tolerance"""
    mode, rows, base = survey
    total, shorter = collections.Counter(), collections.Counter()
    for g, c, n, _, _ in rows:
        if g == "A" and c[0] in ("pos", "len", "dist") and c[3] >= 9:
            total[c[0]] += 1
            shorter[c[0]] += n < base["A"]
    shares = {f: shorter[f] / total[f] for f in ("pos", "len", "dist")}
    print(mode_id(mode), {f: round(v, 3) for f, v in shares.items()})
    assert min(shares.values()) >= BITE, (mode, shares)


def test_the_list_is_deterministic_and_pinned():
    bg = pc.BACKGROUND
    assert len(bg) == 64000 and len(set(bg)) == pc.SYMBOLS
    assert len({bg[i:i + 3] for i in range(len(bg) - 2)}) == len(bg) - 2          # no trigram twice: no match of 3 or more
    assert abs(sum(b > 143 for b in bg) / len(bg) - 1 / 3) < 0.05               # a third of it in 9-bit fixed codes
    assert hashlib.sha256(bg).hexdigest() == hashlib.sha256(bytes(pc.permutation(3)[s] for s in pc.de_bruijn(40, 3))).hexdigest()
    assert hashlib.sha256(bg).hexdigest()[:16] == BACKGROUND_SHA
    a = pc.cases_a()
    assert a == pc.cases_a() and len(set(a)) == len(a)
    assert dict(collections.Counter(c[0] for c in a)) == COUNTS_A
    for P in pc.B_PACKETS:
        b = pc.cases_b(P)
        assert b == pc.cases_b(P) and len(set(b)) == len(b)
        assert dict(collections.Counter(c[0] for c in b)) == COUNTS_B[P], P
    # every case keeps its copies inside the input, and planting changes nothing outside them (the lazy echo aside)
    for geometry, cases in [("A", a)] + [(P, pc.cases_b(P)) for P in pc.B_PACKETS]:
        n = pc.size_of(geometry)[1]
        for c in cases[:: 37]:
            d = pc.plant(c, n)
            p, l, dist = c[2:5]
            assert len(d) == n and d[:p] == bg[:p] or len(c) > 5
            assert d[p:p + l] == d[p - dist:p - dist + l]
            if len(c) > 5:
                p2, l2, d2 = c[5]
                assert d[p2:p2 + l2] == d[p2 - d2:p2 - d2 + l2] and d[p + l] != d[p + l - dist]


BACKGROUND_SHA = "3535adb34930fce4"
ANCHORS = (8000, 16384 + 1500)       # offsets in the packet: one in each batch of either packet


def test_oracle_against_the_reference_build(oracle, ref):
    """`pos`, `len` and `start` cases of geometry A whose packet holds the whole copy, source included, at levels 1..3; copies of
    at most 258 bytes only (longer ones can reach the reference's defect D11, which corrupts its memory). The packet's stream is
    the reference's for one of the hash seeds, as in tests/test_oracle_vs_ref.py.

    The reference drops a block's last byte when one of its 16,384-byte batches holds no match at all (defect D3, SURVEY.md
    App. B), which on this background is every batch but the case's own. So for this comparison, and only here, each batch of the
    packet gets an anchor: 8 bytes from distance 100, thousands of bytes from every boundary and from every case's source."""
    P, n = pc.size_of("A")
    checked = 0
    for c in pc.cases_a():
        fam, _, p, l, dist = c[:5]
        if fam not in ("pos", "len", "start") or l > 258 or (p - dist) // P != (p + l - 1) // P:
            continue
        k = p // P
        off, ln = k * P, min(P, n - k * P)
        b = bytearray(pc.plant(c, n))
        for a in ANCHORS:
            b[off + a:off + a + 8] = b[off + a - 100:off + a - 92]
        d = bytes(b)
        for lvl in (1, 2, 3):
            want = oracle.packet(d, lvl, off, ln, k == 1)
            assert any(want == ref.packet(d, lvl, off, ln, k == 1, s) for s in (1, 2, 3)), (c, lvl)
        checked += 1
    assert checked == 2200
