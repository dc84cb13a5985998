"""The point-index decode on the CPU: tests/cxx/inflate_points_harness.cpp restates zz_decode_points_device on the host -- the
builder, zi_points_check, the batches, phase 1 per segment, the tile counts, the rounds, the verdict, the serial path behind a
refusal -- with the rules of zzflate_amd/csrc/zz_inflate_core.h, built with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every
buffer access bounds-checked; out of range aborts), with ONE lane and with 64 simulated lanes. The yardstick is Python's zlib and
the original bytes (tests/points_cases.py). The 64-lane runs cost 64 decodes each, so they take every small case at every
spacing and the large ones at one spacing."""
import ctypes

import pytest

import points_cases as pc
import zzflate_amd as zz

u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp("points"))


@pytest.fixture(scope="module")
def indexes(H):
    """name, spacing -> rows by the harness's builder, each built once"""
    memo = {}

    def get(name, spacing):
        if (name, spacing) not in memo:
            s, fmt, data = pc.case(name)
            rc, rows, n, entries = pc.h_build(H, s, fmt, spacing)
            assert (rc, n, entries) == (0, len(data), len(rows)), (name, spacing)
            memo[name, spacing] = rows
        return memo[name, spacing]
    return get


def check_shape(rows, s, fmt, data):
    assert rows[0] == [0, 0] and rows[-1][1] == len(data)
    assert all(a[0] < b[0] and a[1] <= b[1] for a, b in zip(rows, rows[1:]))
    assert (rows[-1][0] + 7) // 8 == len(s) - pc.header_len(s, fmt) - pc.TRAILER[fmt]


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_case_at_every_spacing(H, indexes, name):
    s, fmt, data = pc.case(name)
    for spacing in pc.SPACINGS:
        rows = indexes(name, spacing)
        check_shape(rows, s, fmt, data)
        if spacing > len(data):
            assert len(rows) == 2, "one segment"
        # a point at the first boundary at or behind every multiple of the spacing: no two points inside one stretch (the last
        # row is the stream's end, not such a point)
        if spacing > 1:
            assert all(a[1] // spacing < b[1] // spacing for a, b in zip(rows[:-1], rows[1:-1]))
        # every segment alone, with the true 32 KiB in front of it, is its slice of the data
        assert H.zpt_segments_alone(s, len(s), fmt, pc.flat(rows), len(rows), data, len(data)) == 0, (name, spacing)
        first = None
        for batch in (pc.BATCH, pc.SMALL_BATCH):
            if batch == pc.SMALL_BATCH and any(b[1] - a[1] > batch for a, b in zip(rows, rows[1:])):
                continue                                       # a segment longer than the small batch: the check refuses (see below)
            r = pc.h_decode(H, s, fmt, rows, len(data), batch)
            assert (r.rc, r.path) == (0, pc.PATH_POINTS) and r.out == data, (name, spacing, batch)
            assert r.refused_segments == 0 and not r.check_refused
            if first is None:
                first = r
            else:
                assert r.pending == first.pending, "pending bytes do not depend on the batches"
                if len(data) > batch:
                    assert r.batches > 1
        if len(rows) == 2:
            assert first.pending == 0 and first.rounds == 0, "one segment is the serial path's work: nothing can be pending"


@pytest.mark.parametrize("name", pc.NAMES)
def test_sixty_four_lanes(H, indexes, name):
    s, fmt, data = pc.case(name)
    for spacing in (pc.SPACINGS[:4] if name in pc.SMALL else (32768,)):
        rows = indexes(name, spacing)
        one = pc.h_decode(H, s, fmt, rows, len(data), pc.BATCH, 1)
        r = pc.h_decode(H, s, fmt, rows, len(data), pc.BATCH, 64)
        assert (r.rc, r.path) == (0, pc.PATH_POINTS) and r.out == data, (name, spacing)
        assert (r.pending, r.rounds, r.batches) == (one.pending, one.rounds, one.batches)


def test_a_segment_longer_than_a_batch_goes_to_the_serial_path(H, indexes):
    s, fmt, data = pc.case("alice_l6")
    rows = indexes("alice_l6", 100000)
    assert max(b[1] - a[1] for a, b in zip(rows, rows[1:])) > 50000
    r = pc.h_decode(H, s, fmt, rows, len(data), 50000)
    assert (r.rc, r.path, r.check_refused) == (0, pc.PATH_SERIAL, True) and r.out == data


def test_the_list_meets_its_guards(H, indexes):
    """computed, not assumed: what the list is there to exercise is in it"""
    odd_bits = span_tile = zero_len = 0
    most_in_tile = 0
    mostly_pending = nothing_pending = False
    for name in pc.NAMES:
        s, fmt, data = pc.case(name)
        for spacing in pc.SPACINGS:
            rows = indexes(name, spacing)
            odd_bits += sum(1 for r in rows if r[0] & 7)
            for a, b in zip(rows, rows[1:]):
                zero_len += a[1] == b[1]
                span_tile += b[1] > a[1] and a[1] // pc.TILE != (b[1] - 1) // pc.TILE
            per_tile = {}
            for a, b in zip(rows, rows[1:]):                   # whole segments inside one tile
                if b[1] > a[1] and a[1] // pc.TILE == (b[1] - 1) // pc.TILE:
                    per_tile[a[1] // pc.TILE] = per_tile.get(a[1] // pc.TILE, 0) + 1
            most_in_tile = max([most_in_tile] + list(per_tile.values()))
        r = pc.h_decode(H, s, fmt, indexes(name, 32768), len(data))
        if data and r.pending > 0.9 * len(data) and r.rounds >= 3:
            mostly_pending = True
        if len(data) > 100000 and len(indexes(name, 32768)) > 3 and r.pending == 0:
            nothing_pending = True
    assert odd_bits >= 100, odd_bits
    assert span_tile >= 1 and most_in_tile >= 3 and zero_len >= 1, (span_tile, most_in_tile, zero_len)
    assert mostly_pending, "no case with more than 90 % of its bytes pending and at least 3 rounds"
    assert nothing_pending, "no case of several segments without a pending byte"


@pytest.mark.parametrize("name, spacing", [("alice_l6", 4096), ("alice_mem1", 1), ("mix_mem1", 32768), ("periodic_mem1_raw", 100000)])
def test_lying_indexes_still_give_the_bytes_on_the_serial_path(H, indexes, name, spacing):
    """and none of them gets as far as the checksum: the check refuses it, or a segment's own run does"""
    s, fmt, data = pc.case(name)
    rows = indexes(name, spacing)
    sn = len(s) - pc.header_len(s, fmt) - pc.TRAILER[fmt]
    for kind in pc.LIES:
        bad = pc.lie(rows, kind, sn)
        assert bad != rows
        for lanes in ((1, 64) if name in pc.SMALL and spacing > 1 else (1,)):
            r = pc.h_decode(H, s, fmt, bad, len(data), pc.BATCH, lanes)
            assert (r.rc, r.path) == (0, pc.PATH_SERIAL) and r.out == data, (name, kind)
            assert r.check_refused or r.refused_segments >= 1, (name, kind)
            assert not r.checksum_refused


@pytest.mark.parametrize("name", ["alice_l6", "alice_mem1", "alice_gzip_header", "alice_l0", "alice_raw"])
def test_damaged_streams_get_zlibs_verdict(H, indexes, name):
    s, fmt, data = pc.case(name)
    rows = indexes(name, 4096)                                 # honest, made before the damage
    errors = 0
    for bad in pc.flipped(s) + pc.truncated(s):
        want = pc.zlib_verdict(bad, fmt)
        r = pc.h_decode(H, bad, fmt, rows, len(data) + 100)
        if want is None:
            assert r.rc == zz.E_DATA, name
            errors += 1
        else:
            assert r.rc == 0 and r.out == want, name
    if fmt != pc.RAW:
        assert errors == 200 + len(pc.truncated(s)), "a container's trailer catches what the blocks do not"


def test_capacity_exact_and_one_short(H, indexes):
    for name in ("alice_l6", "alice_l0", "one_zlib"):
        s, fmt, data = pc.case(name)
        rows = indexes(name, 4096)
        r = pc.h_decode(H, s, fmt, rows, len(data))
        assert (r.rc, r.path) == (0, pc.PATH_POINTS) and r.out == data
        # the index's own claim about the length is not evidence: the serial path says "no space" (h_decode checks the guard bytes)
        r = pc.h_decode(H, s, fmt, rows, len(data) - 1)
        assert (r.rc, r.path, r.check_refused) == (zz.E_NOSPACE, pc.PATH_SERIAL, True)


@pytest.mark.parametrize("name", pc.NAMES)
def test_the_librarys_builder_is_the_harnesss_row_for_row(H, indexes, name):
    s, fmt, data = pc.case(name)
    for spacing in pc.SPACINGS:
        points, n = zz.points_index_host(s, fmt, spacing)
        assert n == len(data) and points.dtype.is_floating_point is False and tuple(points.shape) == (len(indexes(name, spacing)), 2)
        assert points.tolist() == indexes(name, spacing), (name, spacing)


def test_the_builders_conventions(H):
    s, fmt, data = pc.case("alice_l6")
    want = pc.h_build(H, s, fmt, 4096)[3]
    for fn in (lambda *a: zz.lib.zz_points_index_host(*a), None):
        for max_entries in (0, 1, want - 1):
            entries, n = u64(7), u64(7)
            buf = (u64 * (2 * want))(*([0xEE] * (2 * want)))
            if fn:
                rc = fn(s, len(s), fmt, 4096, buf, max_entries, ctypes.byref(entries), ctypes.byref(n))
            else:
                rc = H.zpt_build(s, len(s), fmt, 4096, buf, max_entries, ctypes.byref(entries), ctypes.byref(n))
            assert (rc, entries.value, n.value) == (zz.E_NOSPACE, want, len(data))
            assert list(buf) == [0xEE] * (2 * want), "nothing is written when the rows do not fit"
    # an invalid stream, a preset dictionary
    import zlib
    bad = bytearray(s); bad[len(s) // 2] ^= 0x10
    co = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=b"hello world")
    fdict = co.compress(b"hello world, hello") + co.flush()
    for stream, code in ((bytes(bad), zz.E_DATA), (s[:-1], zz.E_DATA), (s + b"\x00", zz.E_DATA), (b"", zz.E_DATA), (fdict, zz.E_UNSUPPORTED)):
        entries, n = u64(7), u64(7)
        buf = (u64 * 4096)()
        assert zz.lib.zz_points_index_host(stream, len(stream), fmt, 4096, buf, 2048, ctypes.byref(entries), ctypes.byref(n)) == code
        assert (entries.value, n.value) == (0, 0)
        assert H.zpt_build(stream, len(stream), fmt, 4096, buf, 2048, ctypes.byref(entries), ctypes.byref(n)) == code
    with pytest.raises(zz.ZzFlateError) as e:
        zz.points_index_host(bytes(bad), fmt, 4096)
    assert e.value.code == zz.E_DATA
