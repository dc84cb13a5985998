"""The inflate core (zzflate_amd/csrc/zz_inflate_core.h) on the CPU: tests/cxx/inflate_harness.cpp built with g++
-fsanitize=undefined -DZZ_INFLATE_CHECKED, so every buffer access of the core is bounds-checked (out of range aborts).
Streams from the oracle, Python's zlib and hand-made edge cases decode to their bytes, serially and packet by packet
(phase 1 plus the pointer-jumping resolution of pending bytes); corrupt input gives an error or the exact bytes."""
import ctypes
import os
import random
import shutil
import subprocess
import zlib

import pytest

from conftest import CORPUS, ROOT, Oracle

import zzflate_amd as zz

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_harness.cpp")
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the inflate core harness")
    so = str(tmp_path_factory.mktemp("inflate") / "libinflate_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS],
                   check=True)
    L = ctypes.CDLL(so)
    L.zih_inflate.restype = ctypes.c_int
    L.zih_inflate.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.POINTER(u64)]
    L.zih_packets.restype = ctypes.c_int
    L.zih_packets.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(u64), u64, ctypes.c_void_p, u64,
                              ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.zih_header.restype = ctypes.c_int
    L.zih_header.argtypes = [ctypes.c_int, ctypes.c_char_p, u64]
    return L


def inflate(H, s, fmt, cap):
    out = ctypes.create_string_buffer(max(cap, 1))
    n = u64(0)
    rc = H.zih_inflate(s, len(s), fmt, out, cap, ctypes.byref(n))
    return rc, out.raw[: n.value]


def packets(H, s, fmt, P, index, cap):
    idx = (u64 * len(index))(*index)
    out = ctypes.create_string_buffer(max(cap, 1))
    n = u64(0)
    stats = (u64 * 3)()
    rc = H.zih_packets(s, len(s), fmt, P, idx, len(index), out, cap, ctypes.byref(n), stats)
    return rc, out.raw[: n.value], list(stats)


def corpus(name):
    return open(os.path.join(CORPUS, name), "rb").read()


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


@pytest.mark.parametrize("lvl", range(10))
def test_python_zlib_streams(H, lvl):
    data = corpus("alice29.txt") + corpus("ptt5")[:100000] + corpus("kennedy.xls")[:50000]
    for wbits, fmt in ((15, 0), (31, 1), (-15, 2)):
        co = zlib.compressobj(lvl, zlib.DEFLATED, wbits)
        s = co.compress(data) + co.flush()
        assert inflate(H, s, fmt, len(data)) == (0, data)
        assert inflate(H, s, fmt, len(data) - 1)[0] == zz.E_NOSPACE


@pytest.mark.parametrize("lvl", range(7))
def test_oracle_packet_streams(H, oracle, lvl):
    data = corpus("lcet10.txt")[:120000] + corpus("kennedy.xls")[:60000]
    warms = [0] if lvl in (0, 4, 5, 6) else [0, 4096, 32768]
    for warm in warms:
        for P in (32768, 4096, 1000, 1):
            d = data if P > 1 else data[:3000]
            for fmt in (0, 1, 2):
                s, idx = oracle_packets(oracle, d, fmt, lvl, P, warm)
                assert inflate(H, s, fmt, len(d)) == (0, d), (warm, P, fmt)
                rc, out, _ = packets(H, s, fmt, P, idx, len(d))
                assert (rc, out) == (0, d), (warm, P, fmt)


def test_oracle_sequential_and_ranges_streams(H, oracle):
    data = corpus("lcet10.txt")
    for lvl in (0, 1, 2, 3):
        for fmt in (0, 1, 2):
            assert inflate(H, oracle.encode(data, fmt, lvl), fmt, len(data)) == (0, data)
    for lvl in (0, 2, 3):
        assert inflate(H, oracle.encode_ranges(data, 1, lvl, 7), 1, len(data)) == (0, data)


@pytest.mark.parametrize("kind,lvl", [(zz.GEN_LOG, 2), (zz.GEN_LOG, 3), (zz.GEN_MIX, 2), (zz.GEN_MIX, 3)])
def test_pending_bytes_resolved_packet_by_packet(H, oracle, kind, lvl):
    data = zz.generate_host(kind, 1, 0, 1 << 20)
    for P in (32768, 4096):
        s, idx = oracle_packets(oracle, data, 0, lvl, P)
        rc, out, stats = packets(H, s, 0, P, idx, len(data))
        assert stats[2] > 0, "expected matches that reach in front of a packet's start"
        assert stats[0] > 0 and stats[1] >= 1
        assert rc == 0 and out == data


# ---- hand-made streams -----------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= v << self.n
        self.n += n

    def huff(self, code, n):          # Huffman codes go most significant bit first
        self.put(int(format(code, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    codes, code = [0] * len(lens), 0
    for L in range(1, 16):
        for s, l in enumerate(lens):
            if l == L:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def fixed_lit(b, sym):
    if sym < 144:
        b.huff(0x30 + sym, 8)
    elif sym < 256:
        b.huff(0x190 + sym - 144, 9)
    elif sym < 280:
        b.huff(sym - 256, 7)
    else:
        b.huff(0xC0 + sym - 280, 8)


def zlib_wrap(raw, data):
    return b"\x78\x01" + raw + zlib.adler32(data).to_bytes(4, "big")


def edge_streams():
    rng = random.Random(9)
    out = []
    # distance 32768 and length 258 (fixed code): 32768 random literals, then a 258-byte copy from 32768 back
    lit = bytes(rng.getrandbits(8) for _ in range(32768))
    b = Bits()
    b.put(1, 1); b.put(1, 2)
    for c in lit:
        fixed_lit(b, c)
    fixed_lit(b, 285)                                   # length 258
    b.huff(29, 5); b.put(32768 - 24577, 13)             # distance code 29: 24577 + 13 extra bits
    fixed_lit(b, 256)
    out.append(("dist32768_len258", zlib_wrap(b.bytes(), lit + lit[:258]), lit + lit[:258]))
    # an empty stored block in front of a final fixed block
    b = Bits()
    b.put(0, 1); b.put(0, 2); b.align(); b.put(0, 16); b.put(0xFFFF, 16)
    b.put(1, 1); b.put(1, 2)
    for c in b"xyz":
        fixed_lit(b, c)
    fixed_lit(b, 256)
    out.append(("empty_stored", zlib_wrap(b.bytes(), b"xyz"), b"xyz"))

    # dynamic blocks: literal 'a' (1 bit), end of block and length 3 (2 bits each), ONE distance code (distance 1)
    def dynamic(hclen, cl_lens):
        lens = [0] * 258
        lens[97], lens[256], lens[257] = 1, 2, 2
        b = Bits()
        b.put(1, 1); b.put(2, 2)
        b.put(258 - 257, 5); b.put(0, 5); b.put(hclen - 4, 4)
        order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
        for i in range(hclen):
            b.put(cl_lens.get(order[i], 0), 3)
        clc = canonical([cl_lens.get(s, 0) for s in range(19)])
        seq = lens + [1] if hclen > 4 else [0] * 259        # the distance code: one code of one bit

        def cl(sym):
            b.huff(clc[sym], cl_lens[sym])
        i = 0
        while i < len(seq):
            if seq[i] == 0:
                run = 1
                while i + run < len(seq) and seq[i + run] == 0 and run < 138:
                    run += 1
                if run >= 11:
                    cl(18); b.put(run - 11, 7); i += run
                    continue
            cl(seq[i]); i += 1
        lc = canonical(lens)
        for _ in range(5):
            b.huff(lc[97], 1)
        b.huff(lc[257], 2); b.huff(0, 1)                    # length 3, distance 1
        b.huff(lc[256], 2)
        return b.bytes()
    data = b"a" * 8
    out.append(("single_distance_code_hclen19", zlib_wrap(dynamic(19, {0: 2, 1: 2, 2: 2, 18: 2}), data), data))
    out.append(("hclen18", zlib_wrap(dynamic(18, {0: 2, 1: 2, 2: 2, 18: 2}), data), data))
    # HCLEN 4 can only give lengths 0 and repeats: no end-of-block code, an invalid stream (as zlib says)
    out.append(("hclen4", zlib_wrap(dynamic(4, {0: 1, 18: 1}), data), None))

    # a dynamic block whose literal/length code is ONE one-bit code (end of block) and that has no distance code: an
    # incomplete code zlib accepts, followed by a fixed block with the bytes
    b = Bits()
    b.put(0, 1); b.put(2, 2)
    b.put(0, 5); b.put(0, 5); b.put(19 - 4, 4)
    cl_lens = {0: 2, 1: 2, 18: 1}
    for sym in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        b.put(cl_lens.get(sym, 0), 3)
    clc = canonical([cl_lens.get(x, 0) for x in range(19)])
    b.huff(clc[18], 1); b.put(138 - 11, 7)                  # lengths 0..137: 0
    b.huff(clc[18], 1); b.put(118 - 11, 7)                  # 138..255: 0
    b.huff(clc[1], 2)                                       # 256 (end of block): 1
    b.huff(clc[0], 2)                                       # the one distance length: 0
    b.huff(0, 1)                                            # end of block
    b.put(1, 1); b.put(1, 2)
    for c in b"ok":
        fixed_lit(b, c)
    fixed_lit(b, 256)
    out.append(("one_bit_literal_length_code", zlib_wrap(b.bytes(), b"ok"), b"ok"))
    return out


@pytest.mark.parametrize("name,stream,want", edge_streams(), ids=[e[0] for e in edge_streams()])
def test_hand_made_edge_streams(H, name, stream, want):
    try:
        zl = zlib.decompress(stream)
    except zlib.error:
        zl = None
    assert zl == want, "the hand-made stream is not what it means to be"
    rc, out = inflate(H, stream, 0, 70000)
    if want is None:
        assert rc == zz.E_DATA
    else:
        assert (rc, out) == (0, want)


def test_headers(H):
    assert H.zih_header(0, b"\x78\x9c", 2) == 2
    assert H.zih_header(0, b"\x78\x9d", 2) == -1            # FCHECK
    assert H.zih_header(0, b"\x88\x98", 2) == -1            # CINFO 8
    assert H.zih_header(0, b"\x78\xbb", 2) == -2            # FDICT
    import gzip
    g = gzip.compress(b"hello")
    assert H.zih_header(1, g, len(g)) == 10


def test_corrupt_input_errors_or_exact_bytes(H):
    rng = random.Random(3)
    data = corpus("grammar.lsp")[:2500] + bytes(rng.getrandbits(8) for _ in range(300)) + b"abcabcabc" * 40
    for s, fmt in ((zlib.compress(data, 6), 0), (zlib.compress(data, 1), 0), (__import__("gzip").compress(data), 1)):
        for i in range(len(s)):
            for bit in (0, 3, 7):
                b = bytearray(s); b[i] ^= 1 << bit
                rc, out = inflate(H, bytes(b), fmt, len(data) + 100)
                assert rc != 0 or out == data
        for k in range(len(s)):
            rc, out = inflate(H, s[:k], fmt, len(data) + 100)
            assert rc != 0
    for _ in range(300):
        s = bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 400)))
        for fmt in (0, 1, 2):
            inflate(H, s, fmt, 4096)
            inflate(H, b"\x78\x01" + s, 0, 4096)


def test_corrupt_packets_errors_or_exact_bytes(H, oracle):
    data = corpus("fields.c")[:6000]
    s, idx = oracle_packets(oracle, data, 0, 2, 1000)
    for i in range(2, len(s)):
        b = bytearray(s); b[i] ^= 0x10
        rc, out, _ = packets(H, bytes(b), 0, 1000, idx, len(data))
        assert rc != 0 or out == data
    for j in range(1, len(idx) - 1):                         # a lying index
        bad = list(idx); bad[j] += 1
        rc, out, _ = packets(H, s, 0, 1000, bad, len(data))
        assert rc != 0 or out == data
