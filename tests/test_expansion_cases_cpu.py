"""Guards of the expansion list (tests/expansion_cases.py) that need no GPU: what tests/test_gpu_expansion.py and
tests/test_gpu_dest_edges.py compare the device with is a valid stream of the case's input, the `high` family reaches nine bits a
byte exactly, every packet of the oracle stays inside the per-packet term of zz_bound and comes as close to it as the list claims,
the stored-fallback cells hold both verdicts at neighbouring k, and the capacities swept for the sequential level-1 stream hold its
verdict flips and its one-block threshold.

Smallest slack (per-packet term of zz_bound minus the oracle's packet, over the non-final packets of two bytes or more), as
measured with this list:

    level 0                    0    (len + 10 is met exactly)
    level 1, cold and warm     1    (the closed form of `high`: 1 or 2 by the residue of 9 L mod 8)
    levels 2..6, cold and warm 1    (a stored packet is len + 10, the term len + 11)

The term is never exceeded, final packets and one-byte packets included."""
import zlib

import pytest

import expansion_cases as ec
import zzflate_amd as zz

SLACK = {0: 0, 1: 2, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1}        # the smallest slack is at most this (level 0: exactly this)


def mode_id(m):
    return f"level{m[0]}" + (f"-warm{m[1]}" if m[1] else "")


@pytest.fixture(scope="module", params=ec.GUARD_MODES, ids=mode_id)
def survey(request, oracle):
    """every case once through the oracle in this mode: (mode, [(case, container, stream, [(length, final, packet)])])"""
    lvl, warm = request.param
    rows = []
    for i, c in enumerate(ec.cases()):
        _, n, P = c
        d, fmt = ec.data(c), ec.fmt_of(i)
        s = oracle.encode_packets(d, fmt, lvl, P, warm)
        pk = [(ln, final, ec.oracle_packet(oracle, d, lvl, off, ln, final, warm)) for off, ln, final in ec.packets(n, P)]
        rows.append((c, fmt, s, pk))
    return request.param, rows


def test_oracle_streams_inflate_to_the_input(survey):
    mode, rows = survey
    assert [c for c, fmt, s, _ in rows if not ec.inflates(s, ec.data(c), fmt)] == [], mode


def test_streams_are_their_packets_inside_the_bound(survey):
    """a stream is header, packets, trailer; no packet is larger than the per-packet term and no stream than zz_bound"""
    (lvl, _), rows = survey
    bad = []
    for c, fmt, s, pk in rows:
        if s[ec.HEADER[fmt]:len(s) - ec.TRAILER[fmt]] != b"".join(p for _, _, p in pk):
            bad.append((c, "packets"))
        if len(s) > zz.bound(c[1], fmt, lvl, c[2]):
            bad.append((c, "bound", len(s)))
        bad += [(c, "per packet", ln, len(p)) for ln, _, p in pk if len(p) > ec.per_packet(lvl, ln)]
    assert bad == [], (lvl, bad[:8])


def test_the_list_is_near_the_bound(survey):
    """see the module's docstring: a condition on the list. If the oracle says otherwise the list is to be mended."""
    (lvl, warm), rows = survey
    slack = min(ec.per_packet(lvl, ln) - len(p) for _, _, _, pk in rows for ln, final, p in pk if not final and ln >= 2)
    print(mode_id((lvl, warm)), "smallest slack", slack)
    assert 0 <= slack <= SLACK[lvl] and (lvl != 0 or slack == 0), (lvl, warm, slack)


def test_high_packets_take_nine_bits_a_byte(survey):
    """every packet of every `high` case at level 1, cold and warm: no match was found, and every byte took nine bits"""
    (lvl, warm), rows = survey
    if lvl != 1:
        return
    checked = 0
    for c, _, _, pk in rows:
        if c[0] == "high":
            assert [(ln, final, len(p)) for ln, final, p in pk if len(p) != ec.level1_packet_bytes(ln, final)] == [], (c, warm)
            checked += len(pk)
    assert checked == sum(len(ec.packets(n, P)) for _, n, P in ec.cases("high"))


def test_level0_rule(survey):
    (lvl, _), rows = survey
    if lvl != 0:
        return
    for c, _, _, pk in rows:
        assert all(len(p) == (ln + 5 if final else ln + 10 if ln > 1 else 6) for ln, final, p in pk), c


def test_the_list_is_deterministic():
    h = ec.high(ec.MAX_N)
    assert len(h) == ec.MAX_N == 3 * 32768 + 1 and min(h) >= 144
    assert len({h[i:i + 3] for i in range(len(h) - 2)}) == len(h) - 2            # no trigram twice: no match of 3 or more
    assert ec.high(1000) == h[:1000] and ec.high(300, 2) != h[:300]
    u = ec.uniform(ec.MAX_N)
    assert len(set(u)) == 256 and 0.40 < sum(b >= 144 for b in u) / len(u) < 0.48
    g = ec.geometries()
    assert len(set(g)) == len(g) and max(n for n, _ in g) == ec.MAX_N and all(1 <= P <= 32768 for _, P in g)
    for L in ec.LENGTHS:
        assert {(L, L), (2 * L, L), (3 * L + 1, L), (2 * L - 1, L)} <= set(g)
    assert {(9 * L + 10) % 8 for L in range(1, 18)} == set(range(8))
    assert ec.per_packet(0, 4096) == 4096 + 10 and ec.per_packet(1, 8) == 17 and ec.per_packet(2, 4096) == ec.per_packet(6, 4096) == 4096 + 11


@pytest.mark.parametrize("cell", ec.tip_cells(), ids=lambda c: f"{c[0]}-level{c[1]}-{'final' if c[2] else 'inner'}")
def test_tipping_cells_hold_both_verdicts(oracle, cell):
    """one k in the searched range at which the block goes from stored to dynamic, and only one; the cell is the five k around it,
    and every one of them inflates"""
    L, lvl, final = cell
    v = ec.tip_verdicts(oracle, L, lvl, final)
    assert v[0] and [k for k in range(1, len(v)) if v[k - 1] != v[k]] == [v.index(False)], cell
    tip = ec.tipping(oracle, L, lvl, final)
    ks = [k for k, _ in tip]
    assert len(tip) == 5 and [v[k] for k in ks] == [True, True, False, False, False], (cell, ks)
    for k, d in tip:
        p = ec.oracle_packet(oracle, d, lvl, 0, L, final)
        assert len(p) <= ec.per_packet(lvl, L) and (ec.stored_packet_bytes(L, final) - len(p) > 0) == (not v[k])
        s, P = ec.tip_stream(d, final)
        assert ec.inflates(oracle.encode_packets(s, 2, lvl, P), s, 2) and oracle.encode_packets(s, 2, lvl, P).startswith(p)


def test_both_verdicts_at_every_level(oracle):
    for lvl in ec.TIP_LEVELS:
        for final in (True, False):
            seen = {ec.is_stored(ec.oracle_packet(oracle, d, lvl, 0, L, final), L, final)
                    for L in ec.TIP_LENGTHS for _, d in ec.tipping(oracle, L, lvl, final)}
            assert seen == {True, False}, (lvl, final)


def test_sequential_windows_hold_the_flips_and_the_one_block_threshold(oracle):
    """the capacities tests/test_gpu_dest_edges.py sweeps for the sequential level-1 stream: in the raw container at least two
    changes of verdict (valid stream / the reference stops early), and in every container the capacity from which the stream is
    the roomy one, with the capacity in front of it giving another"""
    for f, n, d in ec.seq_inputs():
        for fmt in (2, 0, 1):
            caps = ec.seq_window(oracle, d, fmt)
            roomy = oracle.encode(d, fmt, 1)
            assert ec.inflates(roomy, d, fmt)
            want = [ec.seq_expected(oracle, d, fmt, c) for c in caps]
            flips = sum((want[i] is None) != (want[i - 1] is None) for i in range(1, len(caps)))
            assert fmt != 2 or flips >= 2, (f, n, flips)
            assert want[0] is None and want[-1] == roomy, (f, n, fmt)
            first = next(i for i in range(len(caps)) if all(w == roomy for w in want[i:]))
            assert first > 0 and caps[first] == ec.one_block_cap(n) + ec.HEADER[fmt], (f, n, fmt, caps[first])
            # (the reference asks nothing of the trailer's room: a stream it would end behind `cap` never comes up here)
            assert all(len(w) <= c for w, c in zip((oracle.encode(d, fmt, 1, cap=c) for c in caps), caps) if ec.inflates(w, d, fmt))


def _valid(b, d, zdict=None):
    try:
        o = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
        return o.decompress(b) == d
    except zlib.error:
        return False


def test_oracle_against_the_reference_build(oracle, ref):
    """every third case and one k of every tipping cell at levels 0..3: the oracle's packet is the compiled reference's for one of
    its hash seeds, as in tests/test_oracle_vs_ref.py -- or, at levels 2 and 3 only, the reference's packet is no encoding of the
    input (a batch without a match drops a byte there: defect D3) and the oracle's is"""
    same = other = 0
    items = [(ec.data(c), c[2]) for c in ec.cases()[::3]]
    items += [ec.tip_stream(ec.tipping(oracle, L, lvl, final)[1 + (L // 64) % 3][1], final) for L, lvl, final in ec.tip_cells() if lvl == 2]
    for d, P in items:
        for lvl in range(4):
            for off, ln, final in ec.packets(len(d), P):
                a = oracle.packet(d, lvl, off, ln, final)
                refs = [ref.packet(d, lvl, off, ln, final, s) for s in (1, 2, 3)]
                if a in refs:
                    same += 1
                else:
                    zd = d[max(0, off - 32768):off] or None
                    assert lvl >= 2 and _valid(a, d[off:off + ln], zd) and not any(_valid(r, d[off:off + ln], zd) for r in refs), (len(d), P, lvl, off)
                    other += 1
    print("the reference's own bytes:", same, "invalid there:", other)
    assert same + other == 4 * sum(len(ec.packets(len(d), P)) for d, P in items) and same > 4 * other
