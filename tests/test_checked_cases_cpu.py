"""The checked range reads' case list and its guards, and the whole procedure on the CPU: tests/cxx/inflate_checked_harness.cpp
built with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access of the core checked), running the range decode with
the sidecar's rules from zz_inflate_core.h -- the fold against the trailer, the widened window, the touched packets summed by one
lane and by 64 and held to their entries. Python's zlib is the yardstick: the sidecars, the folds and every damage case's
decisiveness come from it."""
import ctypes
import os
import shutil
import subprocess
import zlib

import pytest

from conftest import ROOT, Oracle
from range_streams import HAND_P, Bits, packet, ranges_for
import checked_cases as cc

import zzflate_amd as zz

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_checked_harness.cpp")
u64, u32 = ctypes.c_uint64, ctypes.c_uint32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the checked range decode harness")
    so = str(tmp_path_factory.mktemp("inflate_checked") / "libinflate_checked_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS],
                   check=True)
    L = ctypes.CDLL(so)
    L.zch_range.restype = ctypes.c_int
    L.zch_range.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, u32, ctypes.POINTER(u64), u64, ctypes.POINTER(u32), u64, u64, u64,
                            ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), u64, u32]
    L.zch_sidecar.restype = None
    L.zch_sidecar.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, u32, u32, ctypes.POINTER(u32)]
    L.zch_public.restype = u32
    L.zch_public.argtypes = [ctypes.c_int, u32, u32, u32]
    L.zch_partial.restype = ctypes.c_int
    L.zch_partial.argtypes = [ctypes.c_int, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.zch_entries.restype = u64
    L.zch_entries.argtypes = [u64, u32]
    return L


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def read(H, s, fmt, P, index, cks, total_len, first, nbytes, cap=None, batch=0, lanes=1):
    """(rc, bytes or None, [first packet, packets, attempts, pending bytes], out_len); cks None: the unchecked read"""
    idx = (u64 * len(index))(*index)
    ck = None if cks is None else (u32 * len(cks))(*cks)
    cap = min(nbytes, len(index) * P) if cap is None else cap
    out = ctypes.create_string_buffer(b"\xA5" * (cap + 16), cap + 16)
    n = u64(0)
    stats = (u64 * 4)()
    rc = H.zch_range(s, len(s), fmt, P, idx, len(index), ck, total_len, first, nbytes, out, cap, ctypes.byref(n), stats, batch, lanes)
    assert out.raw[cap:] == b"\xA5" * 16
    if rc != 0:
        assert out.raw[:cap] == b"\xA5" * cap                       # the harness copies only what it returns
    return rc, (out.raw[: n.value] if rc == 0 else None), list(stats), n.value


# ---- the case list and its guards --------------------------------------------------------------------------------------------

def test_the_streams_are_what_zlib_reads(oracle):
    names = set()
    for t in cc.streams(oracle):
        names.add(t.name)
        wbits = {0: 15, 1: 31, 2: -15}[t.fmt]
        assert zlib.decompress(t.s, wbits) == t.data, t.name
        assert len(t.idx) == len(t.cks) + 1 == max(1, -(-len(t.data) // t.P)) + 1, t.name
        assert t.idx[0] == 0 and t.idx[-1] == len(cc.body(t)), t.name
    assert len(names) == len(cc.streams(oracle))
    assert {len(cc.stream(oracle, n + "_f0").data) for n in ("empty", "one_full_packet", "P_plus_1")} == {0, 1000, 1001}


def test_host_sidecar_values():
    assert zz.packet_checksums_host(b"", zz.Format.Zlib, 1000) == [1]
    assert zz.packet_checksums_host(b"", zz.Format.Gzip, 1000) == [0] == zz.packet_checksums_host(b"", zz.Format.Deflate, 7)
    d = bytes(range(256)) * 5
    assert zz.packet_checksums_host(d, 0, 500) == [zlib.adler32(d[i: i + 500]) for i in (0, 500, 1000)]
    assert zz.packet_checksums_host(d, 1, 1279) == [zlib.crc32(d[:1279]), zlib.crc32(d[1279:])]
    assert zz.packet_checksums_host(d, 2, 1280) == [zlib.crc32(d)]


def test_sidecars_fold_to_the_trailer(oracle):
    """zlib's per-packet values, turned into start-0 partials and folded with the library's combines, give the stream's trailer"""
    seen = set()
    for t in cc.streams(oracle):
        if t.fmt == 2:
            continue
        seen.add(t.fmt)
        L = len(t.data)
        lens = [max(0, min(t.P, L - k * t.P)) for k in range(len(t.cks))]
        if t.fmt == 0:
            total = 1
            for v, ln in zip(t.cks, lens):
                total = zz.lib.zz_adler32_combine(total, start0(v, ln), ln)
            assert total == zlib.adler32(t.data) == int.from_bytes(t.s[-4:], "big"), t.name
        else:
            total = 0
            for v, ln in zip(t.cks, lens):
                total = zz.lib.zz_crc32_combine(total, v, ln)
            assert total == zlib.crc32(t.data) == int.from_bytes(t.s[-8:-4], "little"), t.name
            assert int.from_bytes(t.s[-4:], "little") == L & 0xFFFFFFFF
    assert seen == {0, 1}


def start0(v, ln):
    """zlib.adler32's value of a packet of ln bytes as the start-0 partial (b << 16) | a"""
    a = ((v & 0xFFFF) - 1) % 65521
    b = ((v >> 16) - ln) % 65521
    return (b << 16) | a


def test_harness_conversions_and_sums(H, oracle):
    for v, ln in ((1, 0), (zlib.adler32(b"abc"), 3), (zlib.adler32(b"\xff" * 32768), 32768), (zlib.adler32(bytes(5000)), 5000)):
        a, b = u32(0), u32(0)
        assert H.zch_partial(1, v, ln, ctypes.byref(a), ctypes.byref(b)) == 1
        assert (b.value << 16) | a.value == start0(v, ln) and H.zch_public(1, a.value, b.value, ln) == v
    a, b = u32(0), u32(0)
    assert H.zch_partial(1, 0xFFF1, 3, ctypes.byref(a), ctypes.byref(b)) == 0       # a half at 65521: no Adler-32 has it
    assert H.zch_partial(1, 0xFFF10001, 3, ctypes.byref(a), ctypes.byref(b)) == 0
    assert H.zch_partial(1, 2, 0, ctypes.byref(a), ctypes.byref(b)) == 0 and H.zch_partial(2, 5, 0, ctypes.byref(a), ctypes.byref(b)) == 0
    assert H.zch_partial(2, 0xDEADBEEF, 9, ctypes.byref(a), ctypes.byref(b)) == 1 and a.value == 0xDEADBEEF
    assert [H.zch_entries(L, 1000) for L in (0, 1, 999, 1000, 1001, 3017)] == [1, 1, 1, 1, 2, 4]
    for t in cc.streams(oracle)[::5] + [cc.stream(oracle, "empty_f0"), cc.stream(oracle, "P_plus_1_f1")]:
        for lanes in (1, 64):
            out = (u32 * len(t.cks))()
            H.zch_sidecar(t.data, len(t.data), t.fmt, t.P, lanes, out)
            assert list(out) == t.cks, (t.name, lanes)
    ff = b"\xff" * (2 * 32768 + 5)                                                  # the Adler edge: sums at their largest
    for fmt in (0, 1):
        out = (u32 * 3)()
        H.zch_sidecar(ff, len(ff), fmt, 32768, 64, out)
        assert list(out) == zz.packet_checksums_host(ff, fmt, 32768)


def test_every_damage_case_is_decisive(oracle):
    cases, made, dropped = cc.damages(oracle)
    assert 10 * dropped <= made, (dropped, made)
    kinds = {c.verdict for c in cases}
    assert kinds == {"packet", "call", "arg"}
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        t = c.stream
        if c.verdict == "packet":
            got = cc.zlib_bytes(t, c.s)
            assert got is not None and len(got) == len(t.data) and c.bad, c.name
            for k in c.bad:                                                         # zlib: the packet's checksum really differs
                f = zlib.adler32 if t.fmt == 0 else zlib.crc32
                assert f(got[k * t.P: (k + 1) * t.P]) != c.cks[k], (c.name, k)
            assert c.cks == t.cks and c.total_len == len(t.data)
        elif c.verdict == "arg":
            assert max(1, -(-c.total_len // t.P)) != len(t.idx) - 1, c.name
        else:
            assert max(1, -(-c.total_len // t.P)) == len(t.idx) - 1, c.name
            assert t.fmt != 2, c.name                                               # a raw stream has no trailer to hold a sidecar to
    lvls = {c.stream.lvl for c in cases if c.verdict == "packet"}
    assert lvls >= {0, 1, 2}


# ---- the procedure on the CPU ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 64])
def test_intact_streams_every_range(H, oracle, lanes):
    for i, t in enumerate(cc.streams(oracle)):
        L = len(t.data)
        if L == 0:
            assert read(H, t.s, t.fmt, t.P, t.idx, t.cks, 0, 0, 5, lanes=lanes)[::3] == (0, 0)
            assert read(H, t.s, t.fmt, t.P, t.idx, t.cks, 0, 0, 0, lanes=lanes)[0] == 0
            continue
        for first, nbytes in ranges_for(L, t.P, i):
            rc, got, stats, _ = read(H, t.s, t.fmt, t.P, t.idx, t.cks, L, first, nbytes, lanes=lanes)
            assert rc == 0 and got == t.data[first: first + nbytes], (t.name, first, nbytes, stats)
            if lanes == 1:
                rc0, got0, stats0, _ = read(H, t.s, t.fmt, t.P, t.idx, None, 0, first, nbytes)
                assert rc0 == 0 and got0 == got and stats0[2] <= stats[2] and stats0[0] >= stats[0], (t.name, first, nbytes)


@pytest.mark.parametrize("lanes", [1, 64])
def test_damage_cases_every_range(H, oracle, lanes):
    for i, c in enumerate(cc.damages(oracle)[0]):
        t = c.stream
        L = len(t.data)
        for first, nbytes in ranges_for(L, t.P, i):
            rc, got, _, n = read(H, c.s, t.fmt, t.P, t.idx, c.cks, c.total_len, first, nbytes, lanes=lanes)
            if c.verdict == "arg":
                assert rc == zz.E_ARG, (c.name, first, nbytes)
                continue
            if c.verdict == "call":
                assert (rc, n) == ((0, 0) if nbytes == 0 else (zz.E_DATA, (1 << 64) - 1)), (c.name, first, nbytes)
                continue
            m = max(0, min(nbytes, L - first))
            k0, k1 = first // t.P, min(len(t.cks), (first + max(nbytes, 1) - 1) // t.P + 1)
            if any(k0 <= k < k1 for k in c.bad):
                assert (rc, n) == (zz.E_DATA, (1 << 64) - 1), (c.name, first, nbytes)
            else:
                assert rc == 0 and got == t.data[first: first + m], (c.name, first, nbytes)
        hit, clean = cc.touching_range(c)
        if c.verdict == "packet":
            assert read(H, c.s, t.fmt, t.P, t.idx, c.cks, c.total_len, *hit, lanes=lanes)[0] == zz.E_DATA, c.name
            rc0, got0, _, _ = read(H, c.s, t.fmt, t.P, t.idx, None, 0, *hit)      # the unchecked rule cannot notice
            assert rc0 == 0 and got0 == cc.zlib_bytes(t, c.s)[hit[0]: hit[0] + hit[1]], c.name


def test_damage_in_a_later_batch(H, oracle):
    t = cc.stream(oracle, "alice29.txt_l0_P1000")
    c = next(c for c in cc.damages(oracle)[0] if c.stream is t and c.bad == [len(t.cks) - 1])
    L = len(t.data)
    for lanes in (1, 64):
        rc, _, _, n = read(H, c.s, t.fmt, t.P, t.idx, c.cks, L, 2000, L, batch=33, lanes=lanes)
        assert (rc, n) == (zz.E_DATA, (1 << 64) - 1)
        rc, got, stats, _ = read(H, c.s, t.fmt, t.P, t.idx, c.cks, L, 2000, L - 2000 - 2 * t.P, batch=33, lanes=lanes)
        assert rc == 0 and got == t.data[2000: L - 2 * t.P] and stats[1] > 66


def widened_window_stream():
    """P = 1000, three packets: literals; literals; then a packet whose bytes [0, 258) copy from one packet back and whose
    bytes from 258 on are literals. With the first attempt's look-back of one packet every byte of packet 2 resolves; packet 1
    starts with a match of distance 1000 into packet 0."""
    import random
    rng = random.Random(99)
    b = Bits()
    index, data = [0], bytearray()
    for k in range(4):
        closing = rng.getrandbits(8)
        if k == 2:
            lits = bytes(data[-HAND_P: -HAND_P + 258]) + bytes(rng.getrandbits(8) for _ in range(HAND_P - 1 - 258))
            body = [(258, HAND_P)] + list(lits[258:])
        elif k == 3:
            lits = bytes(data[-2 * HAND_P: -2 * HAND_P + 258]) + bytes(rng.getrandbits(8) for _ in range(HAND_P - 1 - 258))
            body = [(258, 2 * HAND_P)] + list(lits[258:])
        else:
            lits = bytes(rng.getrandbits(8) for _ in range(HAND_P - 1))
            body = list(lits)
        packet(b, body, closing, k == 3)
        index.append(b.nbytes())
        data += lits + bytes([closing])
    data = bytes(data)
    return b"\x78\x01" + b.bytes() + zlib.adler32(data).to_bytes(4, "big"), index, data


def test_an_external_byte_in_front_of_first_inside_its_packet(H):
    """packet 3's first 258 bytes copy from packet 1, two packets back: with the first look-back (one packet) they are external.
    A read of packet 3 from byte 300 on does not hold them, so the unchecked rule is done after one attempt; the checked rule
    cannot sum packet 3 and takes one more, and both return the same bytes."""
    s, idx, d = widened_window_stream()
    assert zlib.decompress(s) == d
    cks = zz.packet_checksums_host(d, 0, HAND_P)
    first, nbytes = 3 * HAND_P + 300, 200
    rc0, got0, stats0, _ = read(H, s, 0, HAND_P, idx, None, 0, first, nbytes)
    assert rc0 == 0 and got0 == d[first: first + nbytes] and stats0[2] == 1 and stats0[0] == 2
    for lanes in (1, 64):
        rc, got, stats, _ = read(H, s, 0, HAND_P, idx, cks, len(d), first, nbytes, lanes=lanes)
        assert rc == 0 and got == got0 and stats[2] == 2 and stats[0] < 2
    # inside the window the two rules agree
    rc0, got0, stats0, _ = read(H, s, 0, HAND_P, idx, None, 0, 3 * HAND_P + 100, 400)
    rc, got, stats, _ = read(H, s, 0, HAND_P, idx, cks, len(d), 3 * HAND_P + 100, 400)
    assert rc0 == rc == 0 and got0 == got == d[3 * HAND_P + 100: 3 * HAND_P + 500] and stats0[2] == stats[2] == 2
