"""The cases of the decode through a member point index (zz_decode_members_points_device): members_points_cases' files, rows and
lies, with what this call adds -- the verdict zlib's own member loop sets for a file decoded into `cap` bytes (expected), the caps
around every member boundary, the conditions the shapes of the list were chosen for (segment sizes, batches under every file, the
stored member's m* route), the ctypes face of tests/cxx/members_points_decode_harness.cpp and the build of the stand-alone program
tests/cxx/members_points_decode_main.cpp. Shared by the CPU harness's tests (test_members_points_decode_cpu.py) and the device's
(test_gpu_decode_members_points.py)."""
import ctypes
import os
import shutil
import subprocess
import zlib

import members_cases as mc
import members_find_cases as fc
import members_points_cases as C

ROOT = C.ROOT
HARNESS = os.path.join(ROOT, "tests", "cxx", "members_points_decode_harness.cpp")
MAIN = os.path.join(ROOT, "tests", "cxx", "members_points_decode_main.cpp")
u64 = ctypes.c_uint64

OK, NOSPACE, DATA = C.OK, C.NOSPACE, C.DATA
CHUNKS = (64, 1000, 4096, C.BIGGER_THAN_ANY)
BATCHES = (0, 8192, 1024)                                       # batch_bytes; 0: 64 MiB
SPACINGS = (1, 32768)
STORED = "a stored member of more than 64 KiB"
NEAR = "distances near 32,768 across segments"
PLAIN = tuple(n for n in C.valid_cases() if n != STORED)        # the files whose every segment is small at chunk 1,000
ROOMY = 100000                                                  # more than any member of the lists decodes to


def files():
    return {**C.valid_cases(), **C.planted_cases()}


def expected(f, cap):
    """(status, bytes or None): what zlib's member loop sets for the file decoded into `cap` bytes -- members in file order, the
    first that fails decides: NOSPACE if its bytes pass the room before it is found invalid (members_cases.produced), else DATA."""
    if not f:
        return DATA, None
    out, rest = b"", f
    while rest:
        d = zlib.decompressobj(31)
        try:
            got = d.decompress(rest)
            good = d.eof
        except zlib.error:
            good = False
        room = cap - len(out)
        if not good:
            if room >= ROOMY:                                   # (no member of the lists produces that much: produced() is slow)
                return DATA, None
            return (NOSPACE if mc.produced(rest) > room else DATA), None
        if len(got) > room:
            return NOSPACE, None
        out += got
        rest = d.unused_data
    return OK, out


def boundaries(f):
    """the decoded offsets of a valid file's members, the length last"""
    return [off for _, off in fc.true_chain(f)[0]]


def caps_swept(f):
    """every member boundary and the bytes around it, 0, L - 1 and L"""
    b = boundaries(f)
    L = b[-1]
    return sorted({c for x in b for c in (x - 1, x, x + 1) if 0 <= c} | {0, max(L - 1, 0), L})


def segments(rows):
    """[(member, bytes)] of the rows' segments"""
    out, m = [], -1
    for a, b in zip(rows, rows[1:]):
        if a[0] & C.START:
            m += 1
        if not a[0] & C.END:
            out.append((m, b[1] - a[1]))
    return out


def batches(rows, batch_bytes):
    """batches under the rows when every member is dealt: zi_mpd_batch's greedy rule, restated"""
    limit = batch_bytes or (64 << 20)
    segs = [(a[1], b[1]) for a, b in zip(rows, rows[1:]) if not a[0] & C.END]
    n, k0 = 0, 0
    while k0 < len(segs):
        k1 = k0 + 1
        while k1 < len(segs) and segs[k1][1] - segs[k0][0] <= limit:
            k1 += 1
        n += 1
        k0 = k1
    return n


def all_dealt(rows, cap, batch_bytes):
    """no m*: every member ends inside cap and holds no segment longer than a batch"""
    limit = batch_bytes or (64 << 20)
    return rows[-1][1] <= cap and all(n <= limit for _, n in segments(rows))


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def build_harness(directory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the members-points decode harness"
    so = os.path.join(str(directory), "libmembers_points_decode_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    L.zmpd_decode.restype = ctypes.c_int
    L.zmpd_decode.argtypes = [ctypes.c_char_p, u64, ctypes.c_void_p, u64, ctypes.c_void_p, u64, u64, ctypes.c_uint32, ctypes.POINTER(u64),
                              ctypes.c_void_p]
    return L


def build_main(directory):
    """the stand-alone program with the address and undefined-behaviour sanitizers linked in"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the members-points decode program"
    exe = os.path.join(str(directory), "members_points_decode_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", exe, MAIN], check=True)
    return exe


GUARD = 64


class Decoded:
    """a harness call's answer: rc, the bytes (None unless rc is OK) and the stats"""

    def __init__(self, rc, out, stats):
        self.rc, self.out = rc, out
        self.members, self.proven, self.segments, self.batches, self.pending, self.rounds, self.serial, self.turns = stats

    def verdict(self):
        return self.rc, self.out


def h_decode(D, f, rows, cap, batch_bytes=0, lanes=1):
    """the harness over file `f` with `rows` into cap bytes; GUARD bytes behind cap must come back untouched"""
    buf = ctypes.create_string_buffer(b"\xEE" * (cap + GUARD), cap + GUARD)
    n = u64(0)
    stats = (u64 * 8)()
    rc = D.zmpd_decode(f, len(f), C.flat(rows), len(rows), buf, cap, batch_bytes, lanes, ctypes.byref(n), stats)
    assert rc != -100, "the harness contradicts itself (lanes, an iteration cap, a pointer out of range)"
    assert buf.raw[cap:] == b"\xEE" * GUARD, "bytes behind cap were written"
    assert (n.value == (1 << 64) - 1) == (rc != OK)
    st = list(stats)
    assert st[7] <= max(len(rows), 1), "a host loop took more turns than it has rows"
    return Decoded(rc, buf.raw[:n.value] if rc == OK else None, st)


def run_main(exe, path, rows_path, batch_bytes, cap):
    """the stand-alone program: (status, out_len, crc32, stats)"""
    r = subprocess.run([exe, path, rows_path, str(batch_bytes), str(cap)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    head = r.stdout.split()
    assert head[0] == "decode"
    nums = [int(x) for x in head[1:]]
    return nums[0], nums[1], nums[2], nums[3:]


def write_rows(path, rows):
    with open(path, "w") as fh:
        for bit, pos in rows:
            fh.write(f"{bit:x} {pos}\n")
