"""The cases of the point-index decode (zz_points_index_host, zz_decode_points_device): streams this library did not write --
Python's zlib wrote them all -- with the original bytes and zlib's own verdict as the yardstick. Shared by the CPU harness's
tests (test_points_cases_cpu.py) and the device's (test_gpu_decode_points.py); also the harness's ctypes face, so that a
device test sends every stream and index through the bounds-checked host restatement before the device sees it."""
import ctypes
import functools
import os
import random
import shutil
import struct
import subprocess
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = os.path.join(ROOT, "tests", "golden", "corpus")
HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_points_harness.cpp")
u64 = ctypes.c_uint64

ZLIB, GZIP, RAW = 0, 1, 2
WBITS = {ZLIB: 15, GZIP: 31, RAW: -15}
TRAILER = {ZLIB: 4, GZIP: 8, RAW: 0}
SPACINGS = (1, 4096, 32768, 100000, 1 << 40)           # the last is larger than every stream: one segment
TILE = 32768
BATCH = 64 << 20                                       # the device's batch limit (ZZ_INF_BATCH_BYTES)
SMALL_BATCH = 100000                                   # the harness also runs with this one: batch edges inside the 3 MiB case
PATH_SERIAL, PATH_POINTS = 3, 4
GUARD = 64


def corpus(name):
    return open(os.path.join(CORPUS, name), "rb").read()


@functools.lru_cache(maxsize=None)
def data_of(name):
    if name == "alice":
        return corpus("alice29.txt")
    if name == "mix":                                  # about 1.4 MiB
        return corpus("lcet10.txt") + corpus("kennedy.xls")
    if name == "periodic":                             # nearly every byte of every segment copies from the segment before it
        base = bytes(random.Random(1000).getrandbits(8) for _ in range(1000))
        return (base * (3 * 1048576 // 1000 + 1))[: 3 * 1048576]
    if name == "zeros":                                # distance 1
        return bytes(2 * 1048576)
    if name == "empty":
        return b""
    if name == "one":
        return b"z"
    raise KeyError(name)


def gzip_header(extra=b"\x01\x02" * 21, name=b"a file name.txt", hcrc=True):
    h = b"\x1f\x8b\x08" + bytes([4 | 8 | (2 if hcrc else 0)]) + b"\x00\x00\x00\x00\x00\x03"
    h += struct.pack("<H", len(extra)) + extra + name + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def compress(data, fmt, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, long_header=False):
    """`data` as one stream of container `fmt` by zlib.compressobj; flush_every: a Z_SYNC_FLUSH or Z_FULL_FLUSH (in turn, and now
    and then two in a row: an empty stored block behind an empty stored block) every so many bytes; long_header: gzip with
    FNAME, FEXTRA and FHCRC in front of a raw stream"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15 if long_header else WBITS[fmt], mem, strategy)
    out = []
    if flush_every:
        for i, k in enumerate(range(0, len(data), flush_every)):
            out.append(co.compress(data[k: k + flush_every]))
            out.append(co.flush(zlib.Z_SYNC_FLUSH if i % 2 == 0 else zlib.Z_FULL_FLUSH))
            if i % 3 == 0:
                out.append(co.flush(zlib.Z_SYNC_FLUSH))
    else:
        out.append(co.compress(data))
    out.append(co.flush())
    s = b"".join(out)
    if long_header:
        assert fmt == GZIP
        s = gzip_header() + s + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
    return s


# name -> (input, container, compress()'s arguments)
CASES = {
    "alice_l1": ("alice", ZLIB, dict(level=1)),
    "alice_l6": ("alice", ZLIB, dict(level=6)),
    "alice_l9": ("alice", ZLIB, dict(level=9)),
    "alice_mem1": ("alice", ZLIB, dict(level=6, mem=1)),                 # 128-symbol blocks: hundreds of starts at arbitrary bits
    "alice_fixed": ("alice", ZLIB, dict(level=6, strategy=zlib.Z_FIXED)),
    "alice_huffman": ("alice", ZLIB, dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY)),
    "alice_rle": ("alice", ZLIB, dict(level=6, strategy=zlib.Z_RLE)),
    "alice_l0": ("alice", ZLIB, dict(level=0)),                          # stored blocks only
    "alice_flushes": ("alice", ZLIB, dict(level=6, flush_every=3000)),   # empty stored blocks: zero-length segments at spacing 1
    "alice_gzip_header": ("alice", GZIP, dict(level=6, long_header=True)),
    "alice_gzip": ("alice", GZIP, dict(level=9)),
    "alice_raw": ("alice", RAW, dict(level=6)),
    "mix_l1": ("mix", ZLIB, dict(level=1)),
    "mix_l6": ("mix", GZIP, dict(level=6)),
    "mix_l9_raw": ("mix", RAW, dict(level=9)),
    "mix_mem1": ("mix", ZLIB, dict(level=6, mem=1)),
    "periodic_l6": ("periodic", ZLIB, dict(level=6)),
    "periodic_l1": ("periodic", GZIP, dict(level=1)),
    "periodic_mem1_raw": ("periodic", RAW, dict(level=9, mem=1)),
    "zeros_l6": ("zeros", ZLIB, dict(level=6)),
    "zeros_l0": ("zeros", GZIP, dict(level=0)),
    "zeros_rle_raw": ("zeros", RAW, dict(level=6, strategy=zlib.Z_RLE)),
    "empty_zlib": ("empty", ZLIB, dict(level=6)),
    "empty_gzip": ("empty", GZIP, dict(level=6)),
    "empty_raw": ("empty", RAW, dict(level=6)),
    "one_zlib": ("one", ZLIB, dict(level=6)),
    "one_gzip": ("one", GZIP, dict(level=6, long_header=True)),
    "one_raw": ("one", RAW, dict(level=0)),
}
NAMES = tuple(CASES)
SMALL = tuple(n for n in NAMES if CASES[n][0] in ("alice", "empty", "one"))


@functools.lru_cache(maxsize=None)
def case(name):
    """(stream, container, original bytes), the stream verified by zlib itself"""
    inp, fmt, args = CASES[name]
    data = data_of(inp)
    s = compress(data, fmt, **args)
    assert zlib.decompress(s, WBITS[fmt]) == data, name
    return s, fmt, data


def header_len(s, fmt):
    if fmt == ZLIB:
        return 2
    if fmt == RAW:
        return 0
    p, flg = 10, s[3]
    if flg & 4:
        p += 2 + struct.unpack_from("<H", s, p)[0]
    if flg & 8:
        p = s.index(b"\x00", p) + 1
    if flg & 2:
        p += 2
    return p


# ---- lying indexes over valid streams: each must still give the exact bytes, on the serial path ------------------------------
LIES = ("bit_plus_one", "bit_mid_block", "out_off_by_one", "rows_swapped", "row_past_stream", "last_row_dropped", "row_duplicated",
        "row0_not_zero")


def lie(rows, kind, stream_bytes):
    """`rows` (a list of [in_bit, out_byte], at least 4 of them) made to lie in the way `kind` says"""
    r = [list(x) for x in rows]
    k = len(r) // 2
    if kind == "bit_plus_one":
        r[k][0] += 1
    elif kind == "bit_mid_block":
        r[k][0] += (r[k + 1][0] - r[k][0]) // 2
    elif kind == "out_off_by_one":
        r[k][1] += 1
    elif kind == "rows_swapped":
        r[k], r[k + 1] = r[k + 1], r[k]
    elif kind == "row_past_stream":
        r[-1][0] = 8 * stream_bytes + 8
    elif kind == "last_row_dropped":
        r.pop()
    elif kind == "row_duplicated":
        r.insert(k, list(r[k]))
    elif kind == "row0_not_zero":
        r[0] = [1, 0]
    else:
        raise KeyError(kind)
    return r


# ---- damaged streams: honest indexes made before the damage ---------------------------------------------------------------------
def flipped(s, count=200, seed=7):
    """`count` copies of the stream with one seeded bit flipped each"""
    rng = random.Random(seed * 7919 + len(s))
    out = []
    for _ in range(count):
        i, bit = rng.randrange(len(s)), rng.randrange(8)
        b = bytearray(s)
        b[i] ^= 1 << bit
        out.append(bytes(b))
    return out


def truncated(s):
    return [s[:n] for n in sorted({len(s) - 1, len(s) - 3, len(s) - 9, len(s) // 2, len(s) // 7, 12, 3} & set(range(1, len(s))))]


def zlib_verdict(s, fmt):
    """the bytes, or None where zlib refuses the stream (an error, an unfinished stream or bytes behind it)"""
    d = zlib.decompressobj(WBITS[fmt])
    try:
        out = d.decompress(s) + d.flush()
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


# ---- the harness ------------------------------------------------------------------------------------------------------------------
def build_harness(directory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the points harness"
    so = os.path.join(str(directory), "libinflate_points_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    L.zpt_build.restype = ctypes.c_int
    L.zpt_build.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, u64, ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.zpt_decode.restype = ctypes.c_int
    L.zpt_decode.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.c_void_p, u64, u64, ctypes.c_uint32,
                             ctypes.POINTER(u64), ctypes.c_void_p]
    L.zpt_segments_alone.restype = u64
    L.zpt_segments_alone.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.c_char_p, u64]
    return L


def flat(rows):
    return (u64 * (2 * len(rows)))(*[v for r in rows for v in r])


def h_build(H, s, fmt, spacing, max_entries=None):
    """(status, rows, decoded length, entries) by the harness's builder"""
    entries, n = u64(0), u64(0)
    cap = len(s) * 8 + 2 if max_entries is None else max_entries
    buf = (u64 * (2 * max(cap, 1)))()
    rc = H.zpt_build(s, len(s), fmt, spacing, buf, cap, ctypes.byref(entries), ctypes.byref(n))
    rows = [[buf[2 * i], buf[2 * i + 1]] for i in range(entries.value)] if rc == 0 else []
    return rc, rows, n.value, entries.value


class Decoded:
    def __init__(self, rc, out, stats):
        self.rc, self.out = rc, out
        self.pending, self.rounds, self.batches, self.refused_segments = stats[0], stats[1], stats[2], stats[3]
        self.check_refused, self.path, self.checksum_refused = bool(stats[4]), stats[5], bool(stats[6])


def h_decode(H, s, fmt, rows, cap, batch=BATCH, lanes=1):
    """the whole call on the harness; the GUARD bytes behind `cap` must come back untouched"""
    out = ctypes.create_string_buffer(b"\xEE" * (cap + GUARD), cap + GUARD)
    n = u64(0)
    stats = (u64 * 8)()
    rc = H.zpt_decode(s, len(s), fmt, flat(rows), len(rows), out, cap, batch, lanes, ctypes.byref(n), stats)
    assert rc != -100, "the harness contradicts itself (lanes, counts or pointers)"
    assert out.raw[cap:] == b"\xEE" * GUARD, "bytes behind the destination's capacity were written"
    return Decoded(rc, out.raw[: n.value] if rc == 0 else b"", list(stats))
