"""zi_item (zzflate_amd/csrc/zz_inflate_core.h) on the CPU: the routine the batch decoder's kernel (k_inflate_items) runs per
stream -- container header, blocks, trailer and checksum by one group of lanes. tests/cxx/inflate_items_harness.cpp is built
with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED, so every buffer access is bounds-checked (out of range aborts), and runs it
with ONE lane and with 64 simulated lanes (coroutines that meet at the points where a wavefront's lanes depend on each other).
The reference for "decodes correctly" is always the input that the oracle or Python's zlib compressed."""
import ctypes
import gzip
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

from conftest import CORPUS, ROOT, Oracle

import zzflate_amd as zz

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_items_harness.cpp")
u64 = ctypes.c_uint64
GUARD = 64
LANES = (1, 64)
FILES = sorted(os.listdir(CORPUS))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the item harness")
    so = str(tmp_path_factory.mktemp("items") / "libinflate_items_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS],
                   check=True)
    L = ctypes.CDLL(so)
    L.zit_item.restype = ctypes.c_int
    L.zit_item.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.c_uint32, ctypes.POINTER(u64)]
    return L


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def item(H, s, fmt, cap, lanes):
    """(status, decoded bytes); the GUARD bytes behind `cap` must come back untouched"""
    out = ctypes.create_string_buffer(b"\xEE" * (cap + GUARD), cap + GUARD)
    n = u64(0)
    rc = H.zit_item(s, len(s), fmt, out, cap, lanes, ctypes.byref(n))
    assert rc != -100, "the simulated lanes disagree"
    assert out.raw[cap:] == b"\xEE" * GUARD, "bytes behind the destination's capacity were written"
    assert rc == 0 or n.value == 0
    return rc, out.raw[: n.value]


def corpus(name):
    return open(os.path.join(CORPUS, name), "rb").read()


def check_roundtrip(H, s, fmt, data, what):
    for lanes in LANES:
        assert item(H, s, fmt, len(data), lanes) == (0, data), (what, lanes)


@pytest.mark.parametrize("name", FILES)
@pytest.mark.parametrize("lvl", range(4))
def test_oracle_packet_streams_of_the_corpus(H, oracle, name, lvl):
    data = corpus(name)
    for fmt in (0, 1, 2):
        check_roundtrip(H, oracle.encode_packets(data, fmt, lvl, 32768), fmt, data, (name, lvl, fmt))


@pytest.mark.parametrize("lvl", (1, 2, 3, 4, 5, 6))
def test_oracle_warm_windows_and_extended_levels(H, oracle, lvl):
    data = corpus("lcet10.txt")[:120000] + corpus("kennedy.xls")[:60000]
    warms = [0] if lvl >= 4 else [4096, 32768]
    for warm in warms:
        for P in (32768, 4096, 1000):
            for fmt in (0, 1, 2):
                check_roundtrip(H, oracle.encode_packets(data, fmt, lvl, P, warm), fmt, data, (lvl, warm, P, fmt))


def test_oracle_sequential_and_ranges_streams(H, oracle):
    data = corpus("lcet10.txt")[:150000]
    for lvl in (0, 1, 2, 3):
        for fmt in (0, 1, 2):
            check_roundtrip(H, oracle.encode(data, fmt, lvl), fmt, data, ("sequential", lvl, fmt))
    for lvl in (0, 2, 3):
        check_roundtrip(H, oracle.encode_ranges(data, 1, lvl, 7), 1, data, ("ranges", lvl))


@pytest.mark.parametrize("lvl", (0, 1, 6, 9))
def test_python_zlib_streams(H, lvl):
    data = corpus("alice29.txt") + corpus("ptt5")[:100000] + corpus("kennedy.xls")[:50000]
    for wbits, fmt in ((15, 0), (31, 1), (-15, 2)):
        co = zlib.compressobj(lvl, zlib.DEFLATED, wbits)
        s = co.compress(data) + co.flush()
        check_roundtrip(H, s, fmt, data, (lvl, fmt))


def gzip_member(data, extra=None, name=None, comment=None, hcrc=False, level=6):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return h + co.compress(data) + co.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def test_gzip_members_with_every_optional_header_field(H):
    data = corpus("fields.c")
    fields = [dict(), dict(extra=b""), dict(extra=b"\x01\x02" * 300), dict(name=b"file.c"), dict(comment=b"a comment " * 400),
              dict(hcrc=True), dict(extra=b"xy", name=b"n", comment=b"c", hcrc=True), dict(extra=b"q" * 65535, name=b"", hcrc=True)]
    for f in fields:
        s = gzip_member(data, **f)
        assert gzip.decompress(s) == data, "the hand-made member is not what it means to be"
        check_roundtrip(H, s, 1, data, f.keys())
        # a header that runs past the item, and a wrong header CRC
        for lanes in LANES:
            assert item(H, s[:11], 1, len(data), lanes)[0] == zz.E_DATA
        if f.get("hcrc"):
            hl = len(s) - len(gzip_member(data)) + 10
            b = bytearray(s); b[hl - 1] ^= 1
            assert item(H, bytes(b), 1, len(data), 1)[0] == zz.E_DATA


def test_empty_input(H):
    for fmt in (0, 1, 2):
        head = (b"\x78\x01", b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff", b"")[fmt]
        tail = (b"\x00\x00\x00\x01", b"\x00" * 8, b"")[fmt]
        streams = [head + b"\x01\x00\x00\xff\xff" + tail, head + b"\x03\x00" + tail]    # one empty final block: stored, fixed
        # (the oracle, like the reference, wraps NO block for an empty input -- divergence D8; the device writes these two)
        co = zlib.compressobj(6, zlib.DEFLATED, (15, 31, -15)[fmt])
        streams.append(co.compress(b"") + co.flush())
        for s in streams:
            assert zlib.decompress(s, (15, 31, -15)[fmt]) == b"", "not a stream of the empty input"
            for lanes in LANES:
                assert item(H, s, fmt, 0, lanes) == (0, b""), (fmt, s)
                assert item(H, s, fmt, 10, lanes) == (0, b"")
        for lanes in LANES:
            # an item of no bytes at all, or a container around no block, is not a stream
            assert item(H, b"", fmt, 16, lanes)[0] == zz.E_DATA
            assert item(H, head + tail, fmt, 16, lanes)[0] == zz.E_DATA


def test_capacity_exact_and_one_short(H, oracle):
    data = corpus("cp.html")
    streams = [(oracle.encode_packets(data, fmt, lvl, 4096), fmt) for fmt in (0, 1, 2) for lvl in (0, 1, 2)]
    streams += [(zlib.compress(data, 9), 0), (gzip.compress(data), 1)]
    for s, fmt in streams:
        for lanes in LANES:
            assert item(H, s, fmt, len(data), lanes) == (0, data)
            assert item(H, s, fmt, len(data) - 1, lanes) == (zz.E_NOSPACE, b"")     # (item() checks the guard bytes)
            assert item(H, s, fmt, 0, lanes) == (zz.E_NOSPACE, b"")


def test_preset_dictionary_is_unsupported(H):
    co = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=b"hello world")
    s = co.compress(b"hello world, hello") + co.flush()
    assert s[1] & 0x20
    for lanes in LANES:
        assert item(H, s, 0, 100, lanes) == (zz.E_UNSUPPORTED, b"")


def test_wrong_trailers_and_bytes_behind_them(H):
    data = corpus("xargs.1")
    z, g = zlib.compress(data, 6), gzip.compress(data)
    for lanes in LANES:
        for k in range(1, 5):                                   # Adler-32
            b = bytearray(z); b[-k] ^= 0x40
            assert item(H, bytes(b), 0, len(data), lanes)[0] == zz.E_DATA
        for k in range(1, 9):                                   # CRC-32 (the first four) and ISIZE
            b = bytearray(g); b[-k] ^= 0x01
            assert item(H, bytes(b), 1, len(data), lanes)[0] == zz.E_DATA
        for s, fmt in ((z, 0), (g, 1), (z[2:-4], 2)):
            assert item(H, s, fmt, len(data), lanes) == (0, data)
            assert item(H, s + b"\x00", fmt, len(data), lanes)[0] == zz.E_DATA
            assert item(H, s + s, fmt, 2 * len(data), lanes)[0] == zz.E_DATA      # a second member is bytes behind the trailer
            if fmt != 2:
                assert item(H, s[:-1], fmt, len(data), lanes)[0] == zz.E_DATA
        # the wrong container
        assert item(H, z, 1, len(data), lanes)[0] == zz.E_DATA
        assert item(H, g, 0, len(data), lanes)[0] == zz.E_DATA


def test_every_truncation_and_a_flipped_bit_at_every_byte(H):
    rng = random.Random(3)
    data = corpus("grammar.lsp")[:2500] + bytes(rng.getrandbits(8) for _ in range(300)) + b"abcabcabc" * 40
    for s, fmt in ((zlib.compress(data, 6), 0), (zlib.compress(data, 1), 0), (gzip.compress(data), 1)):
        for lanes in LANES:
            for k in range(len(s)):
                assert item(H, s[:k], fmt, len(data) + 100, lanes)[0] == zz.E_DATA, k
            for i in range(len(s)):
                for bit in ((0, 3, 7) if lanes == 1 else (i % 8,)):
                    b = bytearray(s); b[i] ^= 1 << bit
                    rc, out = item(H, bytes(b), fmt, len(data) + 100, lanes)
                    assert rc in (zz.E_DATA, zz.E_NOSPACE, zz.E_UNSUPPORTED) or (rc, out) == (0, data), (i, bit)


def test_random_bytes_end_with_a_status(H):
    rng = random.Random(11)
    for k in range(3000):
        s = bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 400)))
        lanes = 64 if k % 8 == 0 else 1
        for fmt in (0, 1, 2):
            rc, _ = item(H, s, fmt, 4096, lanes)
            assert rc in (0, zz.E_DATA, zz.E_NOSPACE, zz.E_UNSUPPORTED)
        rc, _ = item(H, b"\x78\x01" + s, 0, 4096, lanes)
        assert rc in (0, zz.E_DATA, zz.E_NOSPACE)
        rc, _ = item(H, b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + s, 1, 4096, lanes)
        assert rc in (0, zz.E_DATA, zz.E_NOSPACE)
