"""The range decode's whole procedure on the CPU: tests/cxx/inflate_range_harness.cpp built with g++ -fsanitize=undefined
-DZZ_INFLATE_CHECKED (every buffer access of the core checked; out of range aborts), running phase 1 from the look-back packet,
the rounds with external pointers, the bytes carried between batches and the look-back's growth -- the rules the device takes
from the same header. Every range of an oracle stream equals the slice of its input; hand-made streams pin the attempts."""
import ctypes
import os
import shutil
import subprocess
import zlib

import pytest

from conftest import CORPUS, ROOT, Oracle
from range_streams import HAND_P, hand_stream, ranges_for

import zzflate_amd as zz

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_range_harness.cpp")
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the range decode harness")
    so = str(tmp_path_factory.mktemp("inflate_range") / "libinflate_range_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS],
                   check=True)
    L = ctypes.CDLL(so)
    L.zrh_range.restype = ctypes.c_int
    L.zrh_range.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(u64), u64, u64, u64,
                            ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), u64]
    L.zrh_first_lookback.restype = u64
    L.zrh_first_lookback.argtypes = [ctypes.c_uint32, u64]
    L.zrh_next_lookback.restype = u64
    L.zrh_next_lookback.argtypes = [u64, u64]
    return L


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def oracle_packets(o, data, fmt, lvl, P, warm=0):
    """the oracle's packet-mode stream and its index (from the sizes of its packets)"""
    s = o.encode_packets(data, fmt, lvl, P, warm)
    npk = max(1, (len(data) + P - 1) // P)
    idx, at = [0], 0
    for k in range(npk):
        ln = min(P, len(data) - k * P)
        cap = 2 * ln + 1024
        b = ctypes.create_string_buffer(cap)
        at += o.L.zzo_packet_warm(lvl, data, k * P, ln, int(k == npk - 1), b, cap, warm if lvl < 4 else 0)
        idx.append(at)
    return s, idx


def read(H, s, fmt, P, index, first, nbytes, cap=None, batch=0):
    """(rc, bytes, [first packet, packets, attempts, pending bytes], out_len)"""
    idx = (u64 * len(index))(*index)
    cap = min(nbytes, len(index) * P) if cap is None else cap
    out = ctypes.create_string_buffer(b"\xA5" * (cap + 16), cap + 16)
    n = u64(0)
    stats = (u64 * 4)()
    rc = H.zrh_range(s, len(s), fmt, P, idx, len(index), first, nbytes, out, cap, ctypes.byref(n), stats, batch)
    assert out.raw[cap:] == b"\xA5" * 16
    return rc, (out.raw[: n.value] if rc == 0 else None), list(stats), n.value


def corpus(name):
    return open(os.path.join(CORPUS, name), "rb").read()


def check_ranges(H, s, fmt, P, idx, data, seed, batch=0):
    for first, nbytes in ranges_for(len(data), P, seed):
        rc, got, stats, _ = read(H, s, fmt, P, idx, first, nbytes, batch=batch)
        assert rc == 0 and got == data[first: first + nbytes], (P, fmt, first, nbytes, stats)
        k0 = first // P
        assert stats[0] <= k0 and stats[2] >= 1 and stats[0] + stats[1] > k0


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["alice29.txt", "kennedy.xls"])
def test_oracle_streams_cold(H, oracle, lvl, name):
    data = corpus(name)[:150001]
    for P, fmt in ((32768, 0), (4096, 1), (1000, 2)):
        s, idx = oracle_packets(oracle, data, fmt, lvl, P)
        check_ranges(H, s, fmt, P, idx, data, lvl)


@pytest.mark.parametrize("lvl,warm", [(1, 32768), (2, 32768), (3, 32768), (4, 0), (6, 0)])
def test_oracle_streams_that_reach_far_back(H, oracle, lvl, warm):
    data = corpus("lcet10.txt")[:130000] + corpus("kennedy.xls")[:40000]
    for P in (32768, 4096, 1000):
        s, idx = oracle_packets(oracle, data, 0, lvl, P, warm)
        check_ranges(H, s, 0, P, idx, data, lvl + P)


@pytest.mark.parametrize("P,batch", [(4096, 8), (1000, 33), (1000, 50)])
def test_ranges_longer_than_a_batch(H, oracle, P, batch):
    """batches of at least ZI_BIAS bytes (here: just that): a later batch reads the bytes carried from the one before it, and an
    external byte of a look-back batch stays external in the batches behind it"""
    data = corpus("lcet10.txt")[:200000]
    for lvl, warm in ((2, 0), (6, 0), (2, 32768)):
        s, idx = oracle_packets(oracle, data, 0, lvl, P, warm)
        check_ranges(H, s, 0, P, idx, data, 7, batch=batch)
    s, idx, d = hand_stream("a", 120)
    if P == HAND_P:
        for first, nbytes in ((100 * P + 5, 3000), (40 * P + 100, 70 * P), (119 * P, P)):
            rc, got, stats, _ = read(H, s, 0, P, idx, first, nbytes, batch=batch)
            assert rc == 0 and got == d[first: first + nbytes] and stats[0] == 0


def test_growth_policy(H):
    for P, h0 in ((32768, 1), (1000, 1), (258, 1), (257, 2), (100, 3), (1, 258)):
        assert H.zrh_first_lookback(P, 10 ** 6) == h0                 # one backward extension: 258 bytes
        assert H.zrh_first_lookback(P, 0) == 0 and H.zrh_first_lookback(P, 1) == 1
    for k0 in (1, 2, 3, 5, 17, 40, 1000, 2 ** 40):
        h, steps, work = H.zrh_first_lookback(1000, k0), 0, 0
        while h < k0:
            n = H.zrh_next_lookback(h, k0)
            assert min(k0, 2 * h) <= n <= k0 and n > h                # at least doubling, capped at k0
            work += h
            h, steps = n, steps + 1
        assert h == k0 and steps <= 22 and 3 * work < 4 * h + 1       # the failed attempts' look-backs: a geometric series


def test_hand_made_chain_to_packet_zero(H):
    s, idx, d = hand_stream("a")
    assert zlib.decompress(s) == d
    first = 40 * HAND_P + 100
    rc, got, stats, _ = read(H, s, 0, HAND_P, idx, first, 300)
    assert rc == 0 and got == d[first: first + 300]
    assert stats[0] == 0 and stats[1] == 41 and stats[2] >= 2 and stats[3] > 0
    # the closing stored byte of a packet is a literal: no look-back is needed beyond the first attempt's
    rc, got, stats, _ = read(H, s, 0, HAND_P, idx, 41 * HAND_P - 1, 1)
    assert rc == 0 and got == d[41 * HAND_P - 1: 41 * HAND_P] and stats[2] == 1 and stats[0] == 39
    check_ranges(H, s, 0, HAND_P, idx, d, 5)


def test_hand_made_chain_ends_at_a_literal_packet(H):
    s, idx, d = hand_stream("b")
    assert zlib.decompress(s) == d
    first = 40 * HAND_P + 100
    rc, got, stats, _ = read(H, s, 0, HAND_P, idx, first, 300)
    assert rc == 0 and got == d[first: first + 300]
    assert stats[0] <= 37
    check_ranges(H, s, 0, HAND_P, idx, d, 6)


def test_hand_made_distance_in_front_of_the_stream(H):
    s, idx, d = hand_stream("c", 3)
    with pytest.raises(zlib.error):
        zlib.decompress(s)
    # packet 0 is decoded for every one of these (the range's own packet, or the look-back's)
    for first, nbytes in ((0, 5), (500, 10), (999, 2), (1500, 10)):
        assert read(H, s, 0, HAND_P, idx, first, nbytes)[0] == zz.E_DATA, first


def test_arguments_capacity_and_bad_indexes(H, oracle):
    data = corpus("fields.c")[:6000]
    P = 1000
    s, idx = oracle_packets(oracle, data, 0, 2, P)
    L = len(data)
    assert read(H, s, 0, P, idx, 0, 0)[0] == 0
    assert read(H, s, 0, P, idx, 6 * P, 1)[0] == zz.E_ARG                    # first >= packets * P
    assert read(H, s, 0, P, idx, 5, (1 << 64) - 3)[0] == zz.E_ARG            # first + nbytes overflows
    assert read(H, s, 0, 0, idx, 0, 1)[0] == zz.E_ARG and read(H, s, 0, 32769, idx, 0, 1)[0] == zz.E_ARG
    assert read(H, s, 3, P, idx, 0, 1)[0] == zz.E_ARG and read(H, s, 0, P, idx[:1], 0, 1)[0] == zz.E_ARG
    rc, _, _, n = read(H, s, 0, P, idx, 100, 2000, cap=1999)
    assert rc == zz.E_NOSPACE and n == (1 << 64) - 1
    assert read(H, s, 0, P, idx, L - 10, 100, cap=10)[0] == 0                # clipped: ten bytes fit ten
    assert read(H, b"\x78\xbb" + s[2:], 0, P, idx, 0, 1)[0] == zz.E_UNSUPPORTED
    assert read(H, b"\x79\x01" + s[2:], 0, P, idx, 0, 1)[0] == zz.E_DATA
    assert read(H, s, 0, P, [1] + idx[1:], 0, 1)[0] == zz.E_DATA
    assert read(H, s, 0, P, idx[:-1] + [idx[-1] - 1], 0, 1)[0] == zz.E_DATA
    for j in range(1, len(idx) - 1):                                         # a lying index: refused where the packet is decoded
        bad = list(idx); bad[j] += 1
        rc, got, _, _ = read(H, s, 0, P, bad, (j - 1) * P + 10, P)
        assert rc == zz.E_DATA
    # a flipped length word of a packet's closing stored block (LEN and NLEN no longer match) is refused
    for k in (1, 3):
        b = bytearray(s); b[2 + idx[k + 1] - 3] ^= 0x04
        assert read(H, bytes(b), 0, P, idx, k * P + 1, 10)[0] == zz.E_DATA
