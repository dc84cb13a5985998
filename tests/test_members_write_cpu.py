"""Guards on the case list of zz_encode_members_device (tests/members_write_cases.py) and on its host helpers, without a GPU:
the files the rule composes from the oracle are what zlib and gzip read back, member by member, and the list holds what the
device tests rely on -- stored and compressed members side by side, and a pair of inputs on both sides of the fallback."""
import ctypes
import gzip
import struct

import pytest

import zzflate_amd as zz
import members_cases as mc
import members_write_cases as mw


@pytest.mark.parametrize("level", mw.LEVELS)
def test_expected_files_are_blocked_gzip_files(oracle, level):
    for index, (name, data, B, P, eof) in enumerate(mw.cases(oracle)):
        file, offsets, stored = mw.expected_case(oracle, index, level)
        if file:
            assert mc.yardstick(file) == data, name
            assert gzip.decompress(file) == data, name
        else:
            assert not data and not eof, name
        members = mw.members_of(file)
        blocks = -(-len(data) // B)
        assert len(members) == blocks + (1 if eof else 0), name
        assert [at for at, _ in members[:blocks]] == offsets[:-1] and len(stored) == blocks, name
        assert offsets[-1] == len(file) - (28 if eof else 0), name
        for at, size in members:
            assert size <= 65536, name
            assert file[at:at + 18] == zz.members_header(size), name         # (BSIZE + 1 = the distance to the next member: members_of)
        if eof:
            assert file[-28:] == mc.EOF_BLOCK, name
        assert len(file) <= zz.members_bound(len(data), B, P, eof), name
        if level == 0:
            assert not any(stored), name
            assert len(file) == zz.members_bound(len(data), B, P, eof), name


def test_the_list_holds_stored_and_compressed_members_side_by_side(oracle):
    hits = 0
    for index in range(len(mw.cases(oracle))):
        stored = mw.expected_case(oracle, index, 1)[2]
        hits += any(a != b for a, b in zip(stored, stored[1:]))
    assert hits >= 1


def test_the_threshold_pair_sits_on_both_sides(oracle):
    names = [c[0] for c in mw.cases(oracle)]
    lo, hi = names.index("(8192, 4096), the last r that compresses"), names.index("(8192, 4096), the first r that is stored")
    a, b = mw.cases(oracle)[lo][1], mw.cases(oracle)[hi][1]
    assert len(a) == len(b) and sum(x != y for x, y in zip(a, b)) <= 1           # one byte of text became a random one
    assert mw.expected_case(oracle, lo, 1)[2][0] is False
    assert mw.expected_case(oracle, hi, 1)[2][0] is True
    # on the stored side the body is the level-0 stream, on the other side it is not longer than it
    file, offsets, _ = mw.expected_case(oracle, hi, 1)
    assert offsets[1] - offsets[0] == 26 + mw.stored_stream_bytes(8192, 4096)
    file, offsets, _ = mw.expected_case(oracle, lo, 1)
    assert offsets[1] - offsets[0] <= 26 + mw.stored_stream_bytes(8192, 4096)


def test_gzi_bytes_round_trips_against_the_file(oracle):
    for index, (name, data, B, P, eof) in enumerate(mw.cases(oracle)):
        file, offsets, _ = mw.expected_case(oracle, index, 1)
        parsed = [at for at, _ in mw.members_of(file)]
        if eof:
            parsed = parsed[:-1]
        parsed.append(len(file) - (28 if eof else 0))
        assert parsed == offsets, name
        g = zz.gzi_bytes(parsed, len(data), B)
        count = struct.unpack_from("<Q", g)[0]
        pairs = [struct.unpack_from("<QQ", g, 8 + 16 * i) for i in range(count)]
        assert len(g) == 8 + 16 * count
        assert pairs == [(offsets[i], i * B) for i in range(1, len(offsets) - 1)], name
        # every pair leads to a member that decodes to the input from that offset on
        for c_off, u_off in pairs[:3] + pairs[-1:]:
            size = struct.unpack_from("<H", file, c_off + 16)[0] + 1
            assert mc.yardstick(file[c_off:c_off + size]) == data[u_off:u_off + B], name
    assert zz.gzi_bytes([0], 0, 65280) == struct.pack("<Q", 0)
    with pytest.raises(ValueError):
        zz.gzi_bytes([0, 100], 2 * 65280, 65280)


def test_bound_matches_its_restatement():
    L = zz.lib
    refused = (1 << 64) - 1
    sizes = [(0, 0), (65280, 32768), (65280, 4096), (65280, 1000), (65536, 32768), (65537, 32768), (65500, 32768), (65501, 32768),
             (4096, 4096), (777, 300), (8192, 4096), (1, 1), (2, 1), (100, 1), (65280, 32769), (30000, 30000), (65510, 0), (0, 4096)]
    for B, P in sizes:
        for n in (0, 1, 2, 299, 300, 301, 776, 777, 778, 65279, 65280, 65281, 130560, 196617, (1 << 30) + 5, 1 << 40):
            for flags in (0, 1):
                want = mw.bound(n, B, P, eof=not flags)
                assert L.zz_encode_members_bound(n, B, P, flags) == (refused if want is None else want), (n, B, P, flags)
    # the three pairs the format rule names
    assert mw.stored_stream_bytes(65280, 32768) == 65295 and mw.stored_stream_bytes(65280, 4096) == 65435
    assert mw.stored_stream_bytes(65280, 1000) == 65935 and mw.bound(1, 65280, 1000) is None
    assert zz.members_bound(0) == 28 and zz.members_bound(0, eof=False) == 0
    with pytest.raises(zz.ZzFlateError):
        zz.members_bound(1, 65280, 1000)


def test_members_header():
    assert zz.members_header(28) == mc.EOF_BLOCK[:18]
    assert zz.members_header(65536)[16:] == b"\xff\xff"
    buf = ctypes.create_string_buffer(18)
    assert zz.lib.zz_members_header(0, buf) == zz.E_ARG and zz.lib.zz_members_header(65537, buf) == zz.E_ARG
