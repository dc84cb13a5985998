"""The multi-range decode's whole procedure on the CPU: tests/cxx/inflate_ranges_harness.cpp built with g++ -fsanitize=undefined
-DZZ_INFLATE_CHECKED (every buffer access of the core checked; out of range aborts), running the plan, the waves (with a wave
capacity passed in), phase 1 with segment-relative pointers, the rounds with external pointers, the verdict and the copy -- the
rules the device takes from the same header. Every list of ranges goes in as ONE call; every read equals the slice of the input."""
import ctypes
import os
import shutil
import subprocess
import zlib

import pytest

from conftest import CORPUS, ROOT, Oracle
from range_streams import HAND_P, hand_stream, ranges_for

import zzflate_amd as zz

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_ranges_harness.cpp")
u64 = ctypes.c_uint64
GUARD = 16
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the multi-range decode harness")
    so = str(tmp_path_factory.mktemp("inflate_ranges") / "libinflate_ranges_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS],
                   check=True)
    L = ctypes.CDLL(so)
    L.zrs_ranges.restype = ctypes.c_int
    L.zrs_ranges.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(u64), u64,
                             u64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u64),
                             ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(u64), u64, u64]
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


def call(H, s, fmt, P, index, reads, caps=None, wave=0, limit=0):
    """one call for all `reads` = [(first, nbytes)]: (rc, [bytes or None], [status], [out_len], stats); every destination has a
    guard behind it, which is checked here"""
    k = len(reads)
    span = len(index) * P
    caps = [min(nb, span) for _, nb in reads] if caps is None else caps
    bufs = [ctypes.create_string_buffer(b"\xA5" * (c + GUARD), c + GUARD) for c in caps]
    idx = (u64 * len(index))(*index)
    firsts = (u64 * k)(*[f for f, _ in reads])
    nbytes = (u64 * k)(*[nb for _, nb in reads])
    dsts = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in bufs])
    cps = (u64 * k)(*caps)
    lens = (u64 * k)(*([7] * k))
    status = (ctypes.c_int32 * k)(*([99] * k))
    stats = (u64 * 4)()
    rc = H.zrs_ranges(s, len(s), fmt, P, idx, len(index), k, firsts, nbytes, dsts, cps, lens, status, stats, wave, limit)
    for b, c in zip(bufs, caps):
        assert b.raw[c:] == b"\xA5" * GUARD
    got = [b.raw[: lens[i]] if status[i] == 0 else None for i, b in enumerate(bufs)]
    return rc, got, list(status), list(lens), list(stats)


def corpus(name):
    return open(os.path.join(CORPUS, name), "rb").read()


def check_ranges(H, s, fmt, P, idx, data, seed, wave=0):
    reads = ranges_for(len(data), P, seed)
    rc, got, status, lens, stats = call(H, s, fmt, P, idx, reads, wave=wave)
    assert rc == 0 and status == [0] * len(reads), (P, fmt, rc, status)
    for (first, nbytes), g, m in zip(reads, got, lens):
        assert m == max(0, min(nbytes, len(data) - first)) and g == data[first: first + nbytes], (P, fmt, first, nbytes)
    assert stats[1] >= 1 and stats[3] >= stats[1]
    return got, stats


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["alice29.txt", "kennedy.xls"])
def test_oracle_streams_cold(H, oracle, lvl, name):
    data = corpus(name)[:150001]
    for P, fmt in ((32768, 0), (4096, 1), (1000, 2)):
        s, idx = oracle_packets(oracle, data, fmt, lvl, P)
        check_ranges(H, s, fmt, P, idx, data, lvl)


@pytest.mark.parametrize("lvl,warm", [(2, 32768), (6, 0)])
@pytest.mark.parametrize("name", ["alice29.txt", "kennedy.xls"])
def test_oracle_streams_that_reach_far_back(H, oracle, lvl, warm, name):
    data = corpus(name)[:150001]
    for P, fmt in ((32768, 0), (4096, 1), (1000, 2)):
        s, idx = oracle_packets(oracle, data, fmt, lvl, P, warm)
        check_ranges(H, s, fmt, P, idx, data, lvl + P)


@pytest.mark.parametrize("lvl,warm,P,wave", [(2, 0, 4096, 7), (6, 0, 1000, 40), (2, 32768, 1000, 13), (1, 0, 32768, 1)])
def test_a_small_wave_capacity_gives_the_same_results(H, oracle, lvl, warm, P, wave):
    data = corpus("alice29.txt")[:150001]
    s, idx = oracle_packets(oracle, data, 0, lvl, P, warm)
    one, st1 = check_ranges(H, s, 0, P, idx, data, 3)
    many, stn = check_ranges(H, s, 0, P, idx, data, 3, wave=wave)
    assert many == one and stn[3] > st1[3] and stn[3] >= 2 and stn[:3] == st1[:3]


def hand_reads(P, L):
    """reads that finish in the first attempt (the closing stored byte of a packet is a literal; packet 0 and 1 see packet 0) around
    the one whose chain runs to packet 0"""
    return [(41 * P - 1, 1), (10, 300), (P + 5, 100), (40 * P + 100, 300), (30 * P - 1, 1), (0, P)]


def test_hand_made_chain_to_packet_zero(H):
    s, idx, d = hand_stream("a")
    assert zlib.decompress(s) == d
    reads = hand_reads(HAND_P, len(d))
    for wave in (0, 3):
        rc, got, status, lens, stats = call(H, s, 0, HAND_P, idx, reads, wave=wave)
        assert rc == 0 and status == [0] * len(reads)
        assert got == [d[f: f + nb] for f, nb in reads]
        assert stats[1] > 1 and stats[2] >= 1
        # the reads that finished at once were decoded once: only the retried one comes back
        assert stats[2] == 1
    check_ranges(H, s, 0, HAND_P, idx, d, 5)


def test_hand_made_chain_ends_at_a_literal_packet(H):
    s, idx, d = hand_stream("b")
    assert zlib.decompress(s) == d
    reads = hand_reads(HAND_P, len(d))
    rc, got, status, lens, stats = call(H, s, 0, HAND_P, idx, reads)
    assert rc == 0 and got == [d[f: f + nb] for f, nb in reads]
    assert stats[1] > 1 and stats[2] >= 1
    check_ranges(H, s, 0, HAND_P, idx, d, 6)


def test_hand_made_distance_in_front_of_the_stream(H):
    P = HAND_P
    s, idx, d = hand_stream("c", 44)
    with pytest.raises(zlib.error):
        zlib.decompress(s)
    # packet 0 is decoded for the first four (the read's own packet, the look-back's, or the end of the chain);
    # the closing byte of packet 40 is a literal: its segment is packets 39 and 40, which decode
    reads = [(0, 5), (500, 10), (P + 500, 10), (40 * P + 100, 300), (41 * P - 1, 1)]
    rc, got, status, lens, _ = call(H, s, 0, P, idx, reads)
    assert rc == zz.E_DATA
    assert status == [zz.E_DATA] * 4 + [0] and lens[:4] == [NONE] * 4 and lens[4] == 1 and len(got[4]) == 1


def test_every_status_in_one_call(H, oracle):
    data = corpus("fields.c")[:6000]
    P, L = 1000, 6000
    s, idx = oracle_packets(oracle, data, 0, 2, P)
    reads = [(0, 0), (6 * P, 1), (5, (1 << 64) - 3), (100, 2000), (100, 2000), (L - 10, 100), (0, L), (2500, 100)]
    caps = [0, 10, 10, 1999, 2000, 10, L, 100]
    rc, got, status, lens, _ = call(H, s, 0, P, idx, reads, caps=caps, limit=4)
    assert status == [0, zz.E_ARG, zz.E_ARG, zz.E_NOSPACE, 0, 0, zz.E_UNSUPPORTED, 0]
    assert rc == zz.E_UNSUPPORTED                                   # no ZZ_E_DATA: unsupported goes first
    assert lens == [0, NONE, NONE, NONE, 2000, 10, NONE, 100]
    assert got[4] == data[100:2100] and got[5] == data[L - 10:] and got[7] == data[2500:2600]
    # the precedence of the return value
    assert call(H, s, 0, P, idx, reads[:6], caps=caps[:6])[0] == zz.E_ARG
    assert call(H, s, 0, P, idx, reads[3:6], caps=caps[3:6])[0] == zz.E_NOSPACE
    assert call(H, s, 0, P, idx, reads[4:6], caps=caps[4:6])[0] == 0
    # the per-read limit counts the look-back: packets 1..4 and one in front are five
    assert call(H, s, 0, P, idx, [(1000, 4000)], limit=4)[2] == [zz.E_UNSUPPORTED]
    assert call(H, s, 0, P, idx, [(1000, 4000)], limit=5)[2] == [0]


def test_call_failures_mark_every_read(H, oracle):
    data = corpus("fields.c")[:6000]
    P = 1000
    s, idx = oracle_packets(oracle, data, 0, 2, P)
    reads = [(0, 10), (3000, 10)]
    for bad_s, bad_idx, code in ((b"\x78\xbb" + s[2:], idx, zz.E_UNSUPPORTED), (b"\x79\x01" + s[2:], idx, zz.E_DATA),
                                 (s, [1] + idx[1:], zz.E_DATA), (s, idx[:-1] + [idx[-1] - 1], zz.E_DATA)):
        rc, got, status, lens, _ = call(H, bad_s, 0, P, bad_idx, reads)
        assert rc == code and status == [code, code] and lens == [NONE, NONE]
    assert call(H, s, 0, 0, idx, reads)[0] == zz.E_ARG and call(H, s, 3, P, idx, reads)[0] == zz.E_ARG
    assert call(H, s, 0, P, idx[:1], reads)[0] == zz.E_ARG
    assert call(H, s, 0, P, idx, [])[0] == 0


def test_a_lying_index_entry_spoils_only_the_reads_that_decode_it(H, oracle):
    data = corpus("fields.c")[:6000]
    P = 1000
    s, idx = oracle_packets(oracle, data, 0, 2, P)
    reads = [(k * P + 10, 100) for k in range(6)]
    for j in range(1, len(idx) - 1):
        bad = list(idx); bad[j] += 1                                 # packets j - 1 and j are no longer what the index says
        rc, got, status, lens, _ = call(H, s, 0, P, bad, reads)
        # read k decodes packets k - 1 (the look-back) and k
        spoiled = [k for k in range(6) if {k - 1, k} & {j - 1, j}]
        assert rc == zz.E_DATA and [k for k in range(6) if status[k] == zz.E_DATA] == spoiled, j
        for k in range(6):
            if k not in spoiled:
                assert status[k] == 0 and got[k] == data[k * P + 10: k * P + 110]
    # a flipped length word of a packet's closing stored block
    for k in (1, 3):
        b = bytearray(s); b[2 + idx[k + 1] - 3] ^= 0x04
        rc, got, status, _, _ = call(H, bytes(b), 0, P, idx, reads)
        assert rc == zz.E_DATA and [r for r in range(6) if status[r] != 0] == [k, k + 1]
