"""The cases of the point index built on the device (zz_points_index_device): clean streams by Python's zlib, hand-made streams with
valid block headers PLANTED where no block of the stream starts, edges of the chunking, and damaged streams -- with
zz_points_index_host's rows (through the points harness) and zlib's verdict as the yardsticks. Shared by the CPU harness's tests
(test_points_find_cpu.py) and the device's (test_gpu_points_index.py); also the ctypes face of tests/cxx/points_find_harness.cpp
and the build of the stand-alone program tests/cxx/points_find_main.cpp."""
import ctypes
import functools
import os
import shutil
import struct
import subprocess
import zlib

import points_cases as pc

HARNESS = os.path.join(pc.ROOT, "tests", "cxx", "points_find_harness.cpp")
MAIN = os.path.join(pc.ROOT, "tests", "cxx", "points_find_main.cpp")
u64 = ctypes.c_uint64

OK, NOSPACE, UNSUPPORTED, DATA = 0, -2, -5, -6

# ---- clean streams ---------------------------------------------------------------------------------------------------------------
SMALL = pc.SMALL                                                    # every case over alice, empty and one
LARGE = ("mix_l6", "mix_mem1", "periodic_mem1_raw", "zeros_l6")     # these run at chunk 4,096 only
CLEAN = SMALL + LARGE
BIGGER_THAN_ANY = 1 << 23
CHUNKS = (64, 1000, 4096, 16384, BIGGER_THAN_ANY)                   # 1,000: chunk edges at odd bytes; the last: one chunk


def chunks_of(name):
    return CHUNKS if name in SMALL else (4096,)


# ---- planted streams -------------------------------------------------------------------------------------------------------------
# A non-final STORED block is the first block; its payload is zero bytes up to byte `edge` of D (a chunk edge) and then a complete
# raw DEFLATE stream made at level 6, memLevel 1: many small non-final dynamic blocks, so the payload holds valid headers -- the
# first of them exactly at the chunk's first bit -- that are no block starts of the outer stream. Real dynamic blocks of further
# text follow (memLevel 1 again, so that true candidates follow).
#   merge  the inner stream ends with Z_SYNC_FLUSH: the false run lands byte-aligned exactly where the outer stored block ends
#          and goes on along the true chain -- its links hold from there on, but its byte count is wrong
#   final  the inner stream ends with its own final block in mid-stream
#   two    two such stored blocks in a row
PLANTED = {  # name -> (variant, edge, the chunk sizes it is built for)
    "merge_8000": ("merge", 8000, (1000,)), "final_8000": ("final", 8000, (1000,)), "two_8000": ("two", 8000, (1000,)),
    "merge_8192": ("merge", 8192, (4096,)), "final_8192": ("final", 8192, (4096,)), "two_8192": ("two", 8192, (4096,)),
}


def _raw(data, end):
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    return co.compress(data) + co.flush(end)


def _stored(payload):
    assert len(payload) <= 65535
    return b"\x00" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload


@functools.lru_cache(maxsize=None)
def planted(name):
    """(stream, container, original bytes, planted bits counted from the first DEFLATE byte)"""
    variant, edge, _ = PLANTED[name]
    text = pc.corpus("alice29.txt")
    inner = _raw(text[:12000], zlib.Z_SYNC_FLUSH if variant == "merge" else zlib.Z_FINISH)
    blocks, data, bits, at = [], b"", [], 0
    for k in range(2 if variant == "two" else 1):
        start = at + 5                                             # the payload's first byte in D
        first = (start + edge - 1) // edge * edge if k else edge   # the next chunk edge
        payload = bytes(first - start) + inner
        blocks.append(_stored(payload)); data += payload; bits.append(8 * first)
        at += 5 + len(payload)
    tail = text[12000:60000]
    d = b"".join(blocks) + _raw(tail, zlib.Z_FINISH)
    data += tail
    s = b"\x78\x9c" + d + struct.pack(">I", zlib.adler32(data))
    assert zlib.decompress(s) == data, name
    return s, pc.ZLIB, data, tuple(bits)


# ---- damaged streams -------------------------------------------------------------------------------------------------------------
DAMAGED = ("alice_l6", "alice_mem1")


@functools.lru_cache(maxsize=None)
def damaged(name):
    s, fmt, _ = pc.case(name)
    return tuple(pc.flipped(s, 200)) + tuple(pc.truncated(s)), fmt


# ---- helpers over D ----------------------------------------------------------------------------------------------------------------
def deflate_of(s, fmt):
    """D: the bytes behind the container header, trailer included"""
    return s[pc.header_len(s, fmt):]


def block_type(d, bit):
    """(BFINAL, BTYPE) at `bit` of d"""
    v = int.from_bytes(d[bit // 8: bit // 8 + 2] + b"\x00\x00", "little") >> (bit % 8)
    return v & 1, (v >> 1) & 3


def dynamic_starts(d, rows):
    """the bits of the rows (all but the last) where a non-final dynamic block starts"""
    return [b for b, _ in rows[:-1] if block_type(d, b) == (0, 2)]


# ---- the harness -------------------------------------------------------------------------------------------------------------------
def build_harness(directory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the points-find harness"
    so = os.path.join(str(directory), "libpoints_find_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    L.zpf_index.restype = ctypes.c_int
    L.zpf_index.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, u64, u64, u64, ctypes.c_uint32, ctypes.c_void_p, u64,
                            ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.c_void_p]
    L.zpf_candidates.restype = ctypes.c_int64
    L.zpf_candidates.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, u64, ctypes.c_uint32, ctypes.c_void_p, u64]
    L.zpf_rules.restype = ctypes.c_int64
    L.zpf_rules.argtypes = [ctypes.c_char_p, u64, ctypes.c_uint32, ctypes.c_void_p, u64, ctypes.POINTER(u64)]
    return L


def build_main(directory):
    """the stand-alone program with the address and undefined-behaviour sanitizers linked in"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the points-find program"
    exe = os.path.join(str(directory), "points_find_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", exe, MAIN], check=True)
    return exe


class Found:
    def __init__(self, rc, rows, out_len, entries, stats):
        self.rc, self.rows, self.out_len, self.entries = rc, rows, out_len, entries
        self.candidates, self.dropped, self.rounds, self.jobs = stats

    def key(self):
        return self.rc, self.rows, self.out_len, self.entries, self.candidates, self.dropped, self.rounds


def h_index(H, s, fmt, chunk, spacing=1, limit=0, lanes=1, max_entries=None):
    """the whole call on the harness"""
    cap = len(s) // chunk + 3 if max_entries is None else max_entries
    buf = (u64 * (2 * max(cap, 1)))()
    entries, n = u64(0), u64(0)
    stats = (u64 * 4)()
    rc = H.zpf_index(s, len(s), fmt, chunk, spacing, limit, lanes, buf, cap, ctypes.byref(entries), ctypes.byref(n), stats)
    assert rc != -100, "the harness contradicts itself (lanes, or a chain that does not close)"
    rows = [[buf[2 * i], buf[2 * i + 1]] for i in range(entries.value)] if rc == OK else []
    return Found(rc, rows, n.value, entries.value, list(stats))


def h_candidates(H, s, fmt, chunk, lanes=1):
    cap = len(s) // chunk + 3
    buf = (u64 * cap)()
    n = H.zpf_candidates(s, len(s), fmt, chunk, lanes, buf, cap)
    assert 0 <= n <= cap, n
    return [buf[i] for i in range(n)]


def run_main(exe, path, fmt, chunk, spacing=1, limit=0):
    """the stand-alone program over the stream in the file `path`: a Found"""
    r = subprocess.run([exe, path, str(fmt), str(chunk), str(spacing), str(limit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    head = [int(x) for x in lines[0].split()]
    rows = [[int(x) for x in ln.split()] for ln in lines[1:] if ln]
    return Found(head[0], rows, head[2], head[1], head[3:7])
