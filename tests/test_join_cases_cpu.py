"""Guards of the join list (tests/join_cases.py) that need no GPU: what tests/test_gpu_join.py compares the kernels with is a
valid stream of the case's input in every container, with the trailer zlib computes; the packets of the cases that cross a
round of the size scan differ in size; every boundary the list is for is crossed, by computation from the cases -- and the
host's checksum entry points and the batch decoder's item routine (bounds-checked, tests/cxx/inflate_items_harness.cpp) meet
zlib on 0xFF data at the lengths where their reductions matter."""
import ctypes
import functools
import os
import shutil
import subprocess
import zlib

import pytest

import join_cases as jc
import zzflate_amd as zz
from conftest import ROOT

M = jc.ADLER_MOD
u64 = ctypes.c_uint64


@functools.lru_cache(maxsize=None)
def packet_sizes(oracle, c, lvl):
    d, k = jc.data(c), jc.npk(c)
    return [len(oracle.packet(d, lvl, i * c.P, min(c.P, c.n - i * c.P), i == k - 1)) for i in range(k)]


# ---- the streams ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grp", ["len", "mod", "part", "crc", "round", "batch"])
def test_expected_streams_inflate_in_every_container(oracle, grp):
    """zlib takes every expected stream whole, trailer included; and the trailer is the one zlib's own checksums give"""
    bad = []
    for c in (jc.batch_items() if grp == "batch" else jc.group(grp)):
        d = jc.data(c)
        for lvl in c.levels:
            for fmt in (0, 1, 2):
                s = oracle.encode_packets(d, fmt, lvl, c.P)
                t = jc.trailer(d, fmt)
                if not (jc.inflates(s, d, fmt) and s.startswith(jc.HEADER[fmt]) and s.endswith(t)):
                    bad.append((jc.case_id(c), lvl, fmt))
    assert bad == []


def test_the_list_is_deterministic():
    assert jc.cases() == jc.CASES and len(set(jc.CASES)) == len(jc.CASES)
    for c in jc.CASES[::7] + jc.batch_items():
        d = jc.data(c)
        assert len(d) == c.n and d == jc.data(c)
        if c.family == "ff":
            assert d.count(0xFF) == c.n
        if c.family == "ffnoise":
            assert set(d) <= {0xFE, 0xFF} and (c.n < 64 or len(set(d)) == 2)
        if c.family == "impulse":
            assert d.count(0) == c.n - 1 and d[c.arg] == 0xFF
    # an impulse pins one position's weight: b - n = 255 * (bytes from it to the end)
    c = jc.Case("x", "impulse", 1000, 64, 123, ())
    assert jc.partial(jc.data(c), 0) == ((255 * (1000 - 123) % M) << 16) | 255
    assert jc.partial(b"", 0) == 0 and jc.partial(b"", 1) == 0


def test_packet_sizes_vary_where_a_scan_round_is_crossed(oracle):
    """a scan that loses its carry must move bytes, not only relabel equal ones: at levels >= 1 the packets of every case with more
    than 4096 of them take at least three sizes. At P = 3 that cannot be had -- every packet is 9 bytes, and below P = 7 `ffnoise`
    gives two sizes at the most --, so the 65,537 packets of P = 3 have a sibling at P = 7 that does."""
    seen = 0
    for c in jc.group("round"):
        for lvl in c.levels:
            if lvl == 0 or jc.scan_rounds(c) < 2 or c.family != "ffnoise":
                continue
            sizes = set(packet_sizes(oracle, c, lvl)[:-1])
            if c.P == 3:
                assert sizes == {9}
                assert any(o.P == 7 and jc.npk(o) >= jc.npk(c) - 1 and lvl in o.levels for o in jc.group("round"))
                continue
            assert len(sizes) >= 3, (jc.case_id(c), lvl, sizes)
            seen += 1
    assert seen >= 6
    # every count of packets that crosses a scan round has such a case at a level >= 1
    for k in (4097, 8193, 16385, 65537):
        assert any(jc.npk(c) == k and c.family == "ffnoise" and c.P != 3 and max(c.levels) >= 1 for c in jc.group("round")), k
    # the issue's figure: ffnoise at P = 48, level 3, is far from the stored size
    c = next(c for c in jc.group("round") if c.P == 48 and c.family == "ffnoise")
    assert len(oracle.encode_packets(jc.data(c), 2, 3, c.P)) < 0.7 * c.n


# ---- every boundary is crossed: computed from the cases ----------------------------------------------------------------

def test_lengths_around_the_packet_and_the_modulus():
    P = jc.LEN_P
    for fam in ("ff", "ffnoise", "random", "zeros"):
        ns = {c.n for c in jc.group("len") if c.family == fam}
        assert set(range(1, 18)) | {1023, 1024, 1025, P - 1, P, P + 1} <= ns
        assert {jc.last_packet(c) for c in jc.group("len") if c.family == fam and jc.npk(c) > 1} >= {1, P - 1}
        # wave_adler: no trip (below 16 bytes), one, and a second one at P + 16.. -- and the tail loop's every length
        trips = {jc.wave_adler_trips(min(c.n, P)) for c in jc.group("len") if c.family == fam}
        assert {0, 1} <= trips
        assert {c.n & 15 for c in jc.group("len") if c.family == fam} == set(range(16))
    assert 64 * jc.ADLER_INFLIGHT * 16 == P, "P of the `len` group is one trip of wave_adler's loop"
    assert {jc.wave_adler_trips(n) for n in jc.PART_LENGTHS} >= {1, 2, 3, 5}
    pos = {c.arg for c in jc.group("len") if c.family == "impulse"}
    n = jc.LEN_IMPULSE_N
    assert {0, n - 1, 15, 17, P - 1, P, P + 1} <= pos and all(p < n for p in pos)
    for fam in ("ff", "ffnoise"):
        assert {c.n % M for c in jc.group("mod") if c.family == fam} == {0, 1, M - 1}
        assert {M - 1, M, 2 * M} <= {c.n for c in jc.group("mod") if c.family == fam}
        # and the packets behind the first see every "bytes behind" remainder but in the last packet: the fold's r is not 0
        assert all(jc.npk(c) >= 2 for c in jc.group("mod"))


def test_wave_adler_part_rows_and_trips():
    U = jc.L1P_ADLER_U
    assert jc.PART_EDGES[-1] == 3 * 64 * U * 16
    for fam in ("ff", "ffnoise"):
        ns = [c.n for c in jc.group("part") if c.family == fam]
        assert all(n <= 32768 for n in ns)
        for part in range(3):
            rows = {jc.adler_part_rows(n, part) for n in ns}
            assert ({1, 2, 3, 4, U, U + 1} if part == 0 else {0, 1, 2, 3, U}) <= rows, (part, rows)
        assert {jc.adler_part_trips(n, 0) for n in ns} == {1, 2}
        # exactly U rows for every wavefront (one trip each), and the first byte that gives the first wavefront a second trip
        assert [jc.adler_part_rows(jc.PART_EDGES[-1], p) for p in range(3)] == [U, U, U]
        assert jc.PART_EDGES[-1] in ns and jc.PART_EDGES[-1] + 16 in ns
        assert jc.adler_part_trips(jc.PART_EDGES[-1], 0) == 1 and jc.adler_part_trips(jc.PART_EDGES[-1] + 16, 0) == 2
        # a tail behind the last whole chunk (the last wavefront's), and none
        assert {n & 15 for n in ns} >= {0, 1, 15}
    # a full packet: the wavefronts take 11, 11 and 10 rows, two trips each
    assert [jc.adler_part_rows(32768, p) for p in range(3)] == [11, 11, 10]
    pos = {c.arg for c in jc.group("part") if c.family == "impulse"}
    assert {1023, 1024, 2047, 2048, 3071, 3072, jc.PART_EDGES[-1] - 1, jc.PART_EDGES[-1], 0, 32767} <= pos


def test_the_sums_of_a_full_packet_of_ff_have_room():
    """The worst case of every per-lane accumulator, from the loops' own index arithmetic: a packet of 32,768 bytes of 0xFF is the
    most any of them sees, and the list holds it (`mod`, `crc`). A lane's C in wave_adler_part and in wave_adler stays below
    2^32 there -- their 64 bits are headroom, so narrowing C to 32 bits changes no result at any packet size the library takes --
    and a trip of zi_adler_lanes' inner loop, 65,536 steps of at most 65,520 * 255, is 2^24 times below 2^64: a step more or
    less per trip changes no result either. What these sums can get wrong is an index or a reduction, which the cases pin."""
    chunk = 16 * 255                                              # a chunk's byte sum s; its t is 255 * (0 + 1 + .. + 15)
    worst = 0
    for part in range(jc.PARTS):
        rows = jc.adler_part_rows(32768, part)
        for lane in (0, 63):
            worst = max(worst, sum(((r * jc.PARTS + part) * 64 + lane) * 16 * chunk + 255 * 120 for r in range(rows)))
    assert 700e6 < worst < 1 << 32
    one = sum((63 + 64 * j) * 16 * chunk + 255 * 120 for j in range(32768 // 16 // 64))
    assert one < 1 << 32                                          # wave_adler: one wavefront, 32 chunks a lane
    assert 32768 * (32768 * 255) < 1 << 63                        # len * At of a packet
    assert 65537 * 65520 * 255 < 1 << 41
    assert any(c.family == "ff" and c.P == 32768 and c.n >= 32768 for c in jc.group("mod") + jc.group("crc"))


def test_crc_rows_and_paths():
    rows = {P: jc.crc_rows(P) for P in jc.CRC_PACKETS}
    assert rows == {1000: None, 1024: 1, 2048: 2, 3072: 3, 5120: 5, 9216: 9, 32767: None, 32768: 32}
    loops = {P: jc.crc_loops(r) for P, r in rows.items() if r}
    assert loops == {1024: (0, 0), 2048: (0, 1), 3072: (0, 2), 5120: (0, 4), 9216: (1, 0), 32768: (3, 7)}
    for fam in ("ff", "random"):
        cs = [c for c in jc.group("crc") if c.family == fam]
        assert {c.P for c in cs} == set(jc.CRC_PACKETS)
        assert all(jc.npk(c) == 3 and jc.last_packet(c) == 777 for c in cs)          # two full packets, a short last one
    pos = {c.arg for c in jc.group("crc") if c.family == "impulse"}
    assert {3, 4, 255, 256, 2047, 2048, 8191, 8192, 8192 - 256, 32767, 32768} <= pos


def test_round_edges():
    r = jc.group("round")
    counts = {jc.npk(c) for c in r}
    assert {1023, 1024, 1025, 2049, 4095, 4096, 4097, 8193, 16385, 65537, 65538} <= counts
    assert {jc.reduce_run(c) for c in r} >= {1, 2, 3, 5, 9, 17, 65}                 # k_cks_reduce's packets per thread
    assert {jc.scan_rounds(c) for c in r if max(c.levels) >= 1} >= {1, 2, 3, 5, 17}
    assert any(jc.npk(c) > 2048 for c in r)                                          # the CRC grid (gzip runs on every case)
    assert any(jc.npk(c) > 16384 and 0 in c.levels for c in r)                       # k_encode_l0's grid
    assert any(jc.npk(c) > 65536 and 1 in c.levels for c in r)                       # k_compact's grid
    for c in r:
        assert c.n == (jc.npk(c) - 1) * c.P + jc.last_packet(c) and 1 <= jc.last_packet(c) <= c.P
        if jc.npk(c) <= 1025:
            assert 16 <= c.P <= 64
        elif jc.npk(c) <= 8193:
            assert 16 <= c.P <= 48
        if jc.npk(c) > 65536 and c.P != 256:
            assert max(c.levels) <= 1 and c.P in (3, 7)
        elif jc.npk(c) == 16385:
            assert c.P == 8
    assert {jc.last_packet(c) for c in r} >= {1} and any(jc.last_packet(c) == c.P - 1 for c in r)
    # one case each of levels 2 and 3 at no more than 8193 packets that crosses a scan round
    for lvl in (2, 3):
        assert any(lvl in c.levels and 4096 < jc.npk(c) <= 8193 for c in r)
        assert all(jc.npk(c) <= 8193 for c in r if lvl in c.levels)
    # the sum of the packets' a passes 2^32 in exactly one case: where an unreduced 32-bit fold would show
    big = [c for c in r if c.family == "ff" and jc.npk(c) * ((255 * c.P) % M) >= 1 << 32]
    assert [(c.P, jc.npk(c), c.levels) for c in big] == [(256, 65800, (0,))]
    # the batch: packets per item around the wavefront's 64 lanes (k_batch_finalize strides them; batch_crc_fold's runs of 1..3)
    items = jc.batch_items()
    assert sorted({jc.npk(c) for c in items}) == jc.BATCH_PACKETS == [1, 63, 64, 65, 130]
    assert {-(-jc.npk(c) // 64) for c in items} == {1, 2, 3} and {c.family for c in items} == {"ff", "impulse", "random"}
    assert {jc.last_packet(c) == c.P for c in items} == {True, False}


def test_item_lengths_take_the_outer_loop_twice():
    """zi_adler_lanes: a lane reduces after 65,536 bytes of its own"""
    assert [-(-n // 65536) for n in jc.ITEM_LENGTHS_ONE_LANE] == [1, 1, 2, 4]
    per_lane = -(-jc.ITEM_LENGTH_64_LANES // 64)
    assert per_lane > 65536 and jc.ITEM_LENGTH_64_LANES == 4194304 + 65521 + 3


# ---- the host's checksum entry points --------------------------------------------------------------------------------

def ff_adler(n, start=1):
    """Adler-32 of n bytes of 0xFF on top of `start`, in big integers"""
    a0, b0 = start & 0xFFFF, start >> 16
    a = (a0 + 255 * n) % M
    b = (b0 + n * a0 + 255 * n * (n + 1) // 2) % M
    return (b << 16) | a


def poly_mod(v):
    """v(x) mod the CRC-32 polynomial, plain bit order (bit k = x^k)"""
    G = 0x104C11DB7
    while v.bit_length() > 32:
        v ^= G << (v.bit_length() - 33)
    return v


def rev32(v):
    return int(f"{v:032b}"[::-1], 2)


def crc_shift(crc, nbytes):
    """crc(x) * x^(8 nbytes) mod G on the reflected register, by square and multiply over Python integers"""
    def mul(p, q):
        r = 0
        while q:
            if q & 1:
                r ^= p
            p <<= 1
            q >>= 1
        return poly_mod(r)
    x, e, r = 1 << 8, nbytes, 1
    while e:
        if e & 1:
            r = mul(r, x)
        x = mul(x, x)
        e >>= 1
    return rev32(mul(rev32(crc), r))


def test_host_adler_against_zlib_and_big_integers():
    assert ff_adler(100000) == zlib.adler32(b"\xFF" * 100000)
    for n in (0, 1, 5551, 5552, 5553, 65520, 65521, 65522, 2 * M, (1 << 22) + 77):
        d = b"\xFF" * n
        for start in (1, 0, 0xFFF0FFF0, 0x12345678 % M | ((0x9ABC % M) << 16)):
            assert zz.adler32x(start, d) == zlib.adler32(d, start) == ff_adler(n, start), (n, start)
    d = jc.data(jc.Case("x", "ffnoise", 300001, 1, 3, ()))
    assert zz.adler32x(1, d) == zlib.adler32(d)
    # combine(first, second, len2): second with start value 0
    for n1, n2 in ((0, 1), (1, 0), (5552, 65521), (65521, 65520), (70001, 300001), (1 << 20, (1 << 21) + 5)):
        a, b = b"\xFF" * n1, b"\xFF" * n2
        assert zz.combine(zlib.adler32(a), jc.partial(b, 0), n2) == zlib.adler32(a + b), (n1, n2)
    for n2 in (M - 1, M, M + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1, 1 << 40, (1 << 40) + M):
        for n1 in (0, 1, 65520, 1 << 33):
            first, whole = ff_adler(n1), ff_adler(n1 + n2)
            second = ff_adler(n2, 0)
            assert zz.combine(first, second, n2) == whole, (n1, n2)


def test_host_crc_against_zlib_and_big_integers():
    for n in (0, 1, 3, 4, 5, 1023, 1024, 65535, 65536, (1 << 22) + 77):
        d = b"\xFF" * n
        for start in (0, 0xFFFFFFFF, 0xDEADBEEF):
            assert zz.crc32(d, start) == zlib.crc32(d, start), (n, start)
    d = jc.data(jc.Case("x", "random", 300001, 1, 3, ()))
    assert zz.crc32(d) == zlib.crc32(d)
    assert crc_shift(zlib.crc32(b"abc"), 5) ^ zlib.crc32(bytes(5)) == zlib.crc32(b"abc" + bytes(5))       # the restatement itself
    for n1, n2 in ((0, 1), (1, 0), (1, 1), (1000, 65521), (65536, 32768), (70001, 300001), (1 << 20, (1 << 21) + 5)):
        a, b = b"\xFF" * n1, b"\xFF" * n2
        whole = zlib.crc32(a + b)
        assert zz.crc32_combine(zlib.crc32(a), zlib.crc32(b), n2) == whole, (n1, n2)
        assert crc_shift(zlib.crc32(a), n2) ^ zlib.crc32(b) == whole
    for n2 in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1, 1 << 40, (1 << 40) + 65521):
        for c1, c2 in ((0xFFFFFFFF, 0), (0x12345678, 0x9ABCDEF0), (zlib.crc32(b"\xFF" * 999), 0xFFFFFFFF)):
            assert zz.crc32_combine(c1, c2, n2) == crc_shift(c1, n2) ^ c2, (n2, c1)


# ---- zi_item, bounds-checked, on 0xFF items that take zi_adler_lanes' outer loop more than once -----------------------------

GUARD = 64


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the item harness")
    so = str(tmp_path_factory.mktemp("join_items") / "libinflate_items_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so,
                    os.path.join(ROOT, "tests", "cxx", "inflate_items_harness.cpp")], check=True)
    L = ctypes.CDLL(so)
    L.zit_item.restype = ctypes.c_int
    L.zit_item.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.c_uint32, ctypes.POINTER(u64)]
    return L


def item(H, s, fmt, cap, lanes):
    """(status, decoded bytes); the GUARD bytes behind `cap` must come back untouched"""
    out = ctypes.create_string_buffer(b"\xA5" * (cap + GUARD), cap + GUARD)
    n = u64(0)
    rc = H.zit_item(s, len(s), fmt, out, cap, lanes, ctypes.byref(n))
    assert rc != -100, "the simulated lanes disagree"
    assert out.raw[cap:] == b"\xA5" * GUARD, "bytes behind the destination's capacity were written"
    assert rc == 0 or n.value == 0
    return rc, out.raw[: n.value]


def check_item(H, family, n, fmt, lanes):
    d, s = jc.item_stream(family, n, fmt)
    assert len(s) < 60000 and jc.inflates(s, d, fmt)
    assert item(H, s, fmt, n, lanes) == (0, d), (family, n, fmt, lanes)
    bad = jc.bad_trailers(s, fmt)
    assert len(bad) == 2
    for what, b in bad:
        assert item(H, b, fmt, n, lanes) == (zz.E_DATA, b""), (family, n, fmt, lanes, what)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("family", ["ff", "ffnoise"])
def test_items_one_lane(H, family, fmt):
    for n in jc.ITEM_LENGTHS_ONE_LANE:
        check_item(H, family, n, fmt, 1)


@pytest.mark.parametrize("fmt", [0, 1])
def test_item_of_four_mib_on_64_lanes(H, fmt):
    check_item(H, "ff", jc.ITEM_LENGTH_64_LANES, fmt, 64)
