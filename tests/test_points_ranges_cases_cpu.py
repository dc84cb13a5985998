"""Reads through a point index with windows on the CPU: tests/cxx/inflate_points_ranges_harness.cpp restates
zz_points_windows_host and the whole of zz_decode_points_ranges_device on the host with the rules of
zzflate_amd/csrc/zz_inflate_core.h, built with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access bounds-checked;
out of range aborts), with ONE lane and with 64 simulated lanes, and once more with a stage of 700 bytes so that waves and big
segments occur on small inputs. The yardstick is the bytes that were compressed (tests/points_ranges_cases.py), and Python's zlib
as an independent witness of the sidecar's format. These are also the guards of the list the device test runs.

One expectation differs from the wording of the list it came from, by the call's own rules: `out_off_by_one` changes the lengths
of the two segments beside the lied row, and the sums are folded over the lengths the index gives -- so for a zlib or gzip stream
the fold no longer gives the trailer and the WHOLE call is E_DATA (no read returns anything: stricter than "exactly the reads
beside the row"). Only a raw stream, which has no trailer, shows the per-segment verdict for that lie."""
import ctypes
import zlib

import pytest

import points_cases as pc
import points_ranges_cases as prc

u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def HP(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp("points_for_ranges"))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return prc.build_harness(tmp_path_factory.mktemp("points_ranges"))


@pytest.fixture(scope="module")
def H700(tmp_path_factory):
    return prc.build_harness(tmp_path_factory.mktemp("points_ranges_700"), prc.SMALL_STAGE)


@pytest.fixture(scope="module")
def sidecars(HP, H):
    """name, spacing -> (rows, windows, sums), each built once: the rows by the points harness's builder, the sidecar by this one's"""
    memo = {}

    def get(name, spacing):
        if (name, spacing) not in memo:
            s, fmt, data = pc.case(name)
            rc, rows, n, entries = pc.h_build(HP, s, fmt, spacing)
            assert (rc, n, entries) == (0, len(data), len(rows)), (name, spacing)
            rc, windows, sums = prc.h_windows(H, s, fmt, rows)
            assert rc == 0, (name, spacing)
            memo[name, spacing] = (rows, windows, sums)
        return memo[name, spacing]
    return get


def public_sum(fmt, b):
    return zlib.adler32(b) if fmt in prc.ADLER_FORMATS else zlib.crc32(b)


def check_call(r, want, what):
    lens, status, outs, code, decoded = want
    assert r.status == status, what
    assert r.lens == lens, what
    assert r.outs == outs, what
    assert r.rc == code, what
    assert r.segments_decoded == decoded, what              # guard (c): the distinct non-empty touched segments, from the rows alone


def deflate_of(s, fmt):
    return s[pc.header_len(s, fmt): len(s) - pc.TRAILER[fmt]]


def zlib_segment(s, fmt, rows, k, window):
    """segment k by zlib itself: a raw inflate from the row's byte with the slot's valid bytes as the dictionary"""
    room = rows[k + 1][1] - rows[k][1]
    d = zlib.decompressobj(-15, zdict=bytes(window))
    try:
        return d.decompress(deflate_of(s, fmt)[rows[k][0] // 8:], room)
    except zlib.error:
        return None


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_case_spacing_and_read(H, sidecars, name):
    s, fmt, data = pc.case(name)
    for spacing in prc.SPACINGS:
        rows, windows, sums = sidecars(name, spacing)
        # the sidecar is what the format says, from the data alone
        for k in range(len(rows) - 1):
            v = prc.valid(rows, k)
            assert windows[(k + 1) * prc.WINDOW - v: (k + 1) * prc.WINDOW] == data[rows[k][1] - v: rows[k][1]], (name, spacing, k)
            assert sums[k] == public_sum(fmt, data[rows[k][1]: rows[k + 1][1]]), (name, spacing, k)
        reads = prc.reads_for(rows)
        want = prc.expect(rows, data, reads)
        r = prc.h_reads(H, s, fmt, rows, windows, sums, reads)
        check_call(r, want, (name, spacing))
        assert r.waves == prc.waves_of(rows, reads) == (1 if data else 0), (name, spacing)
        if name in pc.SMALL or spacing == 4096:             # 64 lanes cost 64 decodes each
            check_call(prc.h_reads(H, s, fmt, rows, windows, sums, reads, lanes=64), want, (name, spacing, 64))


@pytest.mark.parametrize("name", pc.SMALL)
def test_waves_and_big_segments_on_a_small_stage(H700, sidecars, name):
    s, fmt, data = pc.case(name)
    for spacing in prc.SPACINGS:
        rows, windows, sums = sidecars(name, spacing)
        reads = prc.reads_for(rows)
        want = prc.expect(rows, data, reads, stage=prc.SMALL_STAGE)
        r = prc.h_reads(H700, s, fmt, rows, windows, sums, reads)
        check_call(r, want, (name, spacing))
        assert r.waves == prc.waves_of(rows, reads, stage=prc.SMALL_STAGE), (name, spacing)
        if name == "alice_mem1" and spacing == 1:           # 128-symbol blocks: hundreds of segments below 700 bytes
            assert r.waves > 10 and r.segments_decoded > 100
        if spacing > len(data) > prc.SMALL_STAGE:
            assert r.segments_decoded == 0 and prc.UNSUPPORTED in r.status and r.rc == prc.UNSUPPORTED


@pytest.mark.parametrize("name,count", [("alice_flushes", 49), ("alice_mem1", 25), ("mix_l6", 2)])
def test_zlib_reads_the_windows_as_dictionaries(sidecars, name, count):
    """guard (a): zlib as an independent witness of the format"""
    s, fmt, data = pc.case(name)
    rows, windows, sums = sidecars(name, 1)
    ks = prc.aligned_segments(rows)
    assert len(ks) == count
    for k in ks:
        v = prc.valid(rows, k)
        assert zlib_segment(s, fmt, rows, k, windows[(k + 1) * prc.WINDOW - v: (k + 1) * prc.WINDOW]) == data[rows[k][1]: rows[k + 1][1]], (name, k)


def inverted_differs(s, fmt, rows, windows, k):
    v = prc.valid(rows, k)
    w = prc.inverted_slot(windows, rows, k)
    got = zlib_segment(s, fmt, rows, k, w[(k + 1) * prc.WINDOW - v: (k + 1) * prc.WINDOW])
    return got != zlib_segment(s, fmt, rows, k, windows[(k + 1) * prc.WINDOW - v: (k + 1) * prc.WINDOW])


def test_an_inverted_window_is_a_mismatch_not_wrong_bytes(H, sidecars):
    """guard (b): on alice_mem1 every aligned segment uses its window (zlib with the inverted dictionary yields other bytes)"""
    s, fmt, data = pc.case("alice_mem1")
    rows, windows, sums = sidecars("alice_mem1", 1)
    ks = prc.aligned_segments(rows)
    assert len(ks) == 25 and all(inverted_differs(s, fmt, rows, windows, k) for k in ks)
    for k in ks:
        reads = prc.damage_reads(rows, k)
        r = prc.h_reads(H, s, fmt, rows, prc.inverted_slot(windows, rows, k), sums, reads)
        assert r.win_copied[k] > 0, k
        check_call(r, prc.expect(rows, data, reads, bad_segments={k}), k)
        assert r.status[0] == prc.DATA and r.status[1] == prc.OK


def test_a_window_nobody_uses_may_hold_anything(H, sidecars):
    """the counter-case: the aligned segments of alice_flushes behind a full flush do not use their window"""
    s, fmt, data = pc.case("alice_flushes")
    rows, windows, sums = sidecars("alice_flushes", 1)
    ks = prc.aligned_segments(rows)
    unused = [k for k in ks if not inverted_differs(s, fmt, rows, windows, k)]
    assert (len(ks), len(unused)) == (49, 24)
    honest = prc.h_reads(H, s, fmt, rows, windows, sums, [(0, len(data))])
    for k in ks:
        reads = prc.damage_reads(rows, k)
        r = prc.h_reads(H, s, fmt, rows, prc.inverted_slot(windows, rows, k), sums, reads)
        assert (honest.win_copied[k] == 0) == (k in unused), k
        check_call(r, prc.expect(rows, data, reads, bad_segments=set() if k in unused else {k}), k)


@pytest.mark.parametrize("name", prc.LIE_CASES)
def test_a_sums_entry_off_by_one(H, sidecars, name):
    s, fmt, data = pc.case(name)
    rows, windows, sums = sidecars(name, 4096)
    reads = prc.reads_for(rows)
    for k in (0, len(sums) // 2, len(sums) - 1):
        r = prc.h_reads(H, s, fmt, rows, windows, prc.sums_off_by_one(sums, k), reads)
        if fmt == pc.RAW:                                   # no trailer: only the reads that touch the segment
            check_call(r, prc.expect(rows, data, reads, bad_segments={k}), (name, k))
            assert prc.DATA in r.status and prc.OK in r.status
        else:                                               # the fold does not give the trailer: the whole call
            assert r.rc == prc.DATA and set(r.status) == {prc.DATA} and r.segments_decoded == 0, (name, k)


@pytest.mark.parametrize("name", prc.LIE_CASES)
def test_lying_indexes(H, sidecars, name):
    s, fmt, data = pc.case(name)
    for spacing in prc.LIE_SPACINGS[name]:
        rows, windows, sums = sidecars(name, spacing)
        assert len(rows) >= 4
        k = len(rows) // 2
        reads = prc.reads_for(rows)
        for kind in prc.SHAPE_LIES:
            r_, w_, s_ = prc.lied(rows, kind, s, windows, sums)
            assert prc.h_windows(H, s, fmt, r_)[0] == prc.DATA, (name, kind)          # guard (d)
            r = prc.h_reads(H, s, fmt, r_, w_, s_, reads)
            assert r.rc == prc.DATA and set(r.status) == {prc.DATA} and r.segments_decoded == 0, (name, spacing, kind)
        for kind in prc.SEGMENT_LIES:
            r_, w_, s_ = prc.lied(rows, kind, s, windows, sums)
            assert prc.h_windows(H, s, fmt, r_)[0] == prc.DATA, (name, kind)          # guard (d)
            r = prc.h_reads(H, s, fmt, r_, w_, s_, reads)
            if kind == "out_off_by_one" and fmt != pc.RAW:  # the lengths changed, so the fold misses the trailer (see the module's docstring)
                assert r.rc == prc.DATA and set(r.status) == {prc.DATA}, (name, spacing, kind)
                continue
            bad = {j for j in (k - 1, k) if r_[j + 1][1] > r_[j][1]}
            # reads are judged by the lied rows (that is the index the call has); a read that is OK returns the true bytes
            lens, status, outs, code, decoded = prc.expect(r_, data, reads, bad_segments=bad)
            assert r.status == status and r.rc == code and r.segments_decoded == decoded, (name, spacing, kind)
            assert r.lens == lens and r.outs == outs, (name, spacing, kind)
            assert prc.OK in status and prc.DATA in status


@pytest.mark.parametrize("name", ["alice_l6", "alice_gzip_header"])
def test_damaged_streams_with_honest_sidecars(H, sidecars, name):
    s, fmt, data = pc.case(name)
    rows, windows, sums = sidecars(name, 4096)
    reads = prc.reads_for(rows)
    for bad in pc.flipped(s, count=25) + pc.truncated(s):
        assert pc.zlib_verdict(bad, fmt) is None
        assert prc.h_windows(H, bad, fmt, rows)[0] in (prc.DATA, prc.UNSUPPORTED)      # guard (d)
        r = prc.h_reads(H, bad, fmt, rows, windows, sums, reads)
        assert r.status[0] == prc.DATA and r.rc in (prc.DATA, prc.UNSUPPORTED), "the whole-stream read"
        for (first, n), st, out in zip(reads, r.status, r.outs):
            if st == prc.OK:
                assert out == data[first: first + n]


def test_a_distance_in_front_of_the_stream_is_refused_whatever_the_slot_holds(H):
    raw, rows, windows, sums, data = prc.hand_made()
    assert pc.zlib_verdict(raw, pc.RAW) is None
    reads = [(11, 1), (10, 3), (0, 10), (0, 13), (3, 2)]
    r = prc.h_reads(H, raw, pc.RAW, rows, windows, sums, reads)
    check_call(r, prc.expect(rows, data, reads, bad_segments={1}), "hand made")
    assert r.status == [prc.DATA, prc.DATA, prc.OK, prc.DATA, prc.OK]


def crc_of_zeros(n):
    """crc32 of n zero bytes without the bytes: the register after n zero bytes is ~0 * x^(8n) mod P (plain, MSB-first arithmetic)"""
    P = 0x104C11DB7

    def mulmod(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            b >>= 1
            a <<= 1
            if a >> 32:
                a ^= P
        return r

    def rev(v):
        return int(format(v, "032b")[::-1], 2)
    x, e, r = 2, 8 * n, 1
    while e:
        if e & 1:
            r = mulmod(r, x)
        x = mulmod(x, x)
        e >>= 1
    return rev(mulmod(0xFFFFFFFF, r)) ^ 0xFFFFFFFF


def test_the_fold_over_64_bit_lengths(H, sidecars):
    """guard (e): combine only, no data"""
    def fold(fmt, sums, lens):
        v = ctypes.c_uint32(0)
        ok = H.zpr_fold(fmt, (ctypes.c_uint32 * max(len(sums), 1))(*sums), (u64 * max(len(lens), 1))(*lens), len(sums), ctypes.byref(v))
        return ok, v.value
    for name in pc.NAMES:
        s, fmt, data = pc.case(name)
        for spacing in (1, 32768):
            rows, windows, sums = sidecars(name, spacing)
            lens = [b[1] - a[1] for a, b in zip(rows, rows[1:])]
            assert fold(fmt, sums, lens) == (1, public_sum(fmt, data)), (name, spacing)
    # a synthetic list with an entry above 2^32: segments of zero bytes, whose sums have closed forms
    assert crc_of_zeros(1000) == zlib.crc32(bytes(1000)) and crc_of_zeros(0) == 0
    lens = [5, (1 << 32) + 7, 0, 70000, 3]

    def adler_of_zeros(n):
        return ((n % 65521) << 16) | 1
    assert adler_of_zeros(70000) == zlib.adler32(bytes(70000))
    assert fold(pc.ZLIB, [adler_of_zeros(n) for n in lens], lens) == (1, adler_of_zeros(sum(lens)))
    assert fold(pc.GZIP, [crc_of_zeros(n) for n in lens], lens) == (1, crc_of_zeros(sum(lens)))
    # an entry no segment of its length can have
    assert fold(pc.ZLIB, [1, 0xFFF10001], [0, 5])[0] == 0 and fold(pc.ZLIB, [2], [0])[0] == 0 and fold(pc.GZIP, [1], [0])[0] == 0
