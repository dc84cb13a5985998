"""The cases of the member point index (zz_members_points_device): files of gzip members whose
members are LARGE in block starts -- written by zlib with memLevel 1, so that a member of some ten KB holds dozens of small dynamic
blocks -- beside empty, stored, fixed and hand-made members; files with a whole member file PLANTED in a stored block; the member
whose first symbol copies from in front of its first byte; damaged files; rows that are no index. Every file's verdict is
members_cases.yardstick's, zlib's own member loop; the index is held to a pure-Python restatement of the definition (Expect).
Shared by the CPU harness's tests (test_members_points_cpu.py) and the device's (test_gpu_members_points.py); also the ctypes
face of tests/cxx/members_points_harness.cpp and the build of the stand-alone program tests/cxx/members_points_main.cpp."""
import ctypes
import functools
import os
import random
import shutil
import struct
import subprocess
import zlib

import deflate_cases as dc
import members_cases as mc
import members_find_cases as fc
import points_cases as pc
from range_streams import Bits

ROOT = pc.ROOT
HARNESS = os.path.join(ROOT, "tests", "cxx", "members_points_harness.cpp")
MAIN = os.path.join(ROOT, "tests", "cxx", "members_points_main.cpp")
u64 = ctypes.c_uint64

OK, NOSPACE, UNSUPPORTED, DATA = 0, -2, -5, -6
START, END = 1 << 63, 1 << 62
BIGGER_THAN_ANY = 1 << 23
CHUNKS = (64, 1000, 4096)                                       # 1,000: chunk edges at odd bytes
LIMITS = (64, 4096, 0)                                          # the harness's own limit; 0: the definition's


REPAIRED = "block headers stored in front of a member's true blocks"
ABSORBED = "a member whose first block is its chunk's candidate"


def bit_of(v):
    return v & ~(START | END)


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def big(data, level=6):
    """a member written by zlib itself with memLevel 1: a block about every 250 bytes of compressed text"""
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 1)
    return co.compress(data) + co.flush()


def member1(data, level=6, **fields):
    """mc.member (a hand-made header) around memLevel-1 blocks"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 1)
    raw = co.compress(data) + co.flush()
    shell = mc.member(b"", 0, **fields)
    hl = fc.header_len(shell, 0)
    return shell[:hl] + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def ending_at(data, target, level=6):
    """member1 of `data` padded with FEXTRA to exactly `target` bytes"""
    base = len(member1(data, level, extra=b""))
    assert target >= base, (target, base)
    m = member1(data, level, extra=b"\x00" * (target - base))
    assert len(m) == target
    return m


def raw_member(raw, data_crc, isize):
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", data_crc, isize)


def fixed_member(data):
    """one final fixed block of literals"""
    b = Bits()
    blk = dc.Fixed(b, True)
    for c in data:
        blk.sym(c)
    blk.sym(256)
    return raw_member(b.bytes(), zlib.crc32(data), len(data))


def periodic(n, period, seed):
    base = bytes(random.Random(seed).getrandbits(8) for _ in range(period))
    return (base * (n // period + 1))[:n]


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: file}: zlib's member loop accepts every one"""
    rng = random.Random(23)
    alice, fields, cp = mc.corpus("alice29.txt"), mc.corpus("fields.c"), mc.corpus("cp.html")
    a, b, c, d = alice[:40000], alice[40000:75000], alice[75000:110000], alice[110000:145000]
    small = cp[:20000]
    cases = {}
    cases["two large members"] = big(a) + big(b, 1)
    cases["three large members"] = big(a, 9) + big(c) + big(d, 1)
    cases["large members, an empty member and bgzip's last member"] = big(b) + mc.member(b"") + mc.EOF_BLOCK + big(c) + mc.EOF_BLOCK
    cases["FEXTRA, FNAME, FCOMMENT and FHCRC headers"] = (
        member1(d, name=b"d.txt") + member1(a, comment=b"the second") + member1(c, hcrc=True)
        + member1(b, extra=mc.subfield(b"AB", b"hello"), name=b"n", comment=b"c", hcrc=True))
    cases["a stored member of more than 64 KiB"] = big(b) + mc.member(bytes(rng.getrandbits(8) for _ in range(70000)), 0) + big(a[:12000])
    cases["a one-block fixed member"] = big(small) + fixed_member(b"a fixed block of literals, and nothing else") + big(a[:12000], 1)
    # the absorbed case: the member behind a filler of 64,000 bytes begins at a chunk edge (64 and 1,000 divide it), its first
    # block is a non-final dynamic block and the lowest candidate of its chunk
    cases[ABSORBED] = fc.sized(64000, rng)[0] + big(a) + big(c)
    for dd in (-1, 0, 1):
        m1 = ending_at(a[:12000], 8000 + dd)                         # 8,000: an edge of the chunks of 64 and 1,000 bytes; 16,384: of 64 and 4,096
        cases[f"a member end {dd:+d} bytes from a chunk edge"] = m1 + ending_at(small[:9000], 16384 + dd - len(m1)) + big(b[:20000])
    # text whose every stretch of about forty bytes stands 32,700 bytes earlier too: copies from near the window's far edge in
    # every block, so the first bytes of most segments wait for the segment before them
    near = bytearray(alice[:32700] * 3)
    for i in range(32700, len(near), 41):
        near[i] = rng.getrandbits(8)
    cases["distances near 32,768 across segments"] = big(bytes(near)) + big(bytes(near[5000:75000]), 1)
    for name, f in cases.items():
        assert mc.yardstick(f) is not None, name
    return cases


LARGE_MEMBERS = {  # name -> the members (by number) that are large: at least 8 inner rows at chunk 1,000
    "two large members": (0, 1), "three large members": (0, 1, 2), "large members, an empty member and bgzip's last member": (0, 3),
    "FEXTRA, FNAME, FCOMMENT and FHCRC headers": (0, 1, 2, 3), "a stored member of more than 64 KiB": (0,),
    ABSORBED: (1, 2), "distances near 32,768 across segments": (0, 1),
}
# small enough for 64 simulated lanes on every run
SMALL = ("a one-block fixed member", "a member end +0 bytes from a chunk edge")


@functools.lru_cache(maxsize=None)
def planted_cases():
    """a whole two-member file stored inside a stored block of a member: a false header candidate and false block candidates"""
    alice = mc.corpus("alice29.txt")
    inner = big(alice[:20000]) + big(alice[20000:45000], 9)
    assert len(inner) <= 65535
    host = mc.member(inner, 0)
    assert inner in host
    import points_find_cases as pfc
    z, _, data, _ = pfc.planted("merge_8000")                     # a zlib stream: a stored block that holds block headers, then true blocks
    cases = {
        "a member file stored in the middle member": big(alice[50000:70000]) + host + big(alice[70000:90000], 1),
        "a member file stored in the first member": host + big(alice[50000:70000]),
        # the walk lands behind a stored block on a bit that is no candidate: a gap, a repair job, a second round
        REPAIRED: big(alice[50000:70000]) + raw_member(z[2:-4], zlib.crc32(data), len(data)) + big(alice[70000:90000], 1),
    }
    for name, f in cases.items():
        assert mc.yardstick(f) is not None, name
    return cases


def origin_case(dist):
    """(file, the bytes in front of member 2): member 2 is a hand-made fixed block whose first symbol copies ten bytes from
    `dist` back -- from member 1's bytes, which a decoder that counts positions from the file's start would find there. Its
    trailer holds the CRC-32 of exactly those ten bytes."""
    first = mc.text(3000, 4)
    b = Bits()
    blk = dc.Fixed(b, True)
    blk.match(10, dist)
    blk.sym(256)
    wrong = bytes(first[len(first) - dist + (i % dist)] for i in range(10))
    f = big(first) + raw_member(b.bytes(), zlib.crc32(wrong), 10)
    assert mc.yardstick(f) is None
    return f, first


def three_large():
    """(file, members): the damaged cases' good file"""
    alice = mc.corpus("alice29.txt")
    ms = [big(alice[:9000]), big(alice[9000:21000], 1), big(alice[21000:30000], 9)]
    return b"".join(ms), ms


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """{name: (file, what the index call answers: OK, DATA or None for either)}: zlib refuses every one"""
    good, ms = three_large()
    ends = [len(ms[0]), len(ms[0]) + len(ms[1]), len(good)]
    cases = {}

    def flipped(pos):
        f = bytearray(good); f[pos] ^= 1
        return bytes(f)
    for k, nm in enumerate(("the first", "the middle", "the last")):
        cases[f"CRC-32 wrong in {nm} member"] = (flipped(ends[k] - 8), OK)
        cases[f"ISIZE wrong in {nm} member"] = (flipped(ends[k] - 4), DATA)
    for name, pad in (("one byte of garbage", b"\x5a"), ("zero padding", b"\x00" * 7)):
        cases[name + " behind the first trailer"] = (ms[0] + pad + ms[1] + ms[2], DATA)
        cases[name + " behind the file"] = (good + pad, DATA)
    cases["the empty file"] = (b"", DATA)
    for name, (f, _) in cases.items():
        assert mc.yardstick(f) is None, name
    return cases


def truncations():
    f, ms = fc.small_three()
    ends = (len(ms[0]), len(ms[0]) + len(ms[1]))
    return [f[:cut] for cut in range(1, len(f)) if cut not in ends]


LIES = ("bit_plus_one", "out_plus_one", "start_flag_dropped", "end_flag_dropped", "both_flags", "inner_row_flagged", "rows_swapped",
        "end_row_removed", "last_end_row_removed", "another_file")


def lie(rows, kind, other):
    """`rows` of a file with two members or more, large ones, made to lie in the way `kind` says; `other`: another file's rows"""
    r = [list(x) for x in rows]
    inner = [i for i, x in enumerate(r) if not x[0] & (START | END)]
    starts = [i for i, x in enumerate(r) if x[0] & START]
    ends = [i for i, x in enumerate(r) if x[0] & END]
    k = inner[len(inner) // 2]
    if kind == "bit_plus_one":
        r[k][0] += 1
    elif kind == "out_plus_one":
        r[k][1] += 1
    elif kind == "start_flag_dropped":
        r[starts[1]][0] &= ~START
    elif kind == "end_flag_dropped":
        r[ends[0]][0] &= ~END
    elif kind == "both_flags":
        r[ends[0]][0] |= START
    elif kind == "inner_row_flagged":
        r[k][0] |= START
    elif kind == "rows_swapped":
        r[k], r[k + 1] = r[k + 1], r[k]
    elif kind == "end_row_removed":
        del r[ends[0]]
    elif kind == "last_end_row_removed":
        r.pop()
    elif kind == "another_file":
        r = [list(x) for x in other]
    else:
        raise KeyError(kind)
    return r


# ---- the definition, restated --------------------------------------------------------------------------------------------------------
class Expect:
    """What the definition gives for a valid file: the members from zlib's own loop (members_find_cases.true_chain), every block
    boundary of every member from the host builder at spacing 1 (`HP`: the points harness), and the rows: START, the block
    candidates `bc` that are block boundaries of the member, END."""

    def __init__(self, HP, f, hc, bc):
        chain, used = fc.true_chain(f)
        self.index = chain
        self.members = len(used)
        assert hc == fc.candidates(f)
        cand = set(bc)
        self.rows, self.inner, self.absorbed, self.inner_of = [], 0, 0, []
        for (c, off), u in zip(chain[:-1], used):
            first = 8 * (c + fc.header_len(f, c))
            rc, rows, n, _ = pc.h_build(HP, f[c:c + u], pc.GZIP, 1)
            assert rc == 0
            self.rows.append([first | START, off])
            self.absorbed += first in cand
            mine = [[first + b, off + o] for b, o in rows[1:-1] if first + b in cand]
            self.rows += mine
            self.inner += len(mine); self.inner_of.append(len(mine))
            self.rows.append([(first + rows[-1][0]) | END, off + n])
        self.out_len = chain[-1][1]
        self.dropped_headers = len(hc) - self.members
        self.dropped_blocks = len(bc) - self.inner - self.absorbed
        self.dropped = self.dropped_headers + self.dropped_blocks


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def build_harness(directory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the members-points harness"
    so = os.path.join(str(directory), "libmembers_points_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    L.zmp_index.restype = ctypes.c_int
    L.zmp_index.argtypes = [ctypes.c_char_p, u64, u64, u64, u64, ctypes.c_uint32, ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                            ctypes.c_void_p]
    L.zmp_candidates.restype = ctypes.c_int
    L.zmp_candidates.argtypes = [ctypes.c_char_p, u64, u64, ctypes.c_uint32, ctypes.c_void_p, u64, ctypes.c_void_p, u64, ctypes.c_void_p]
    L.zmp_to_index.restype = u64
    L.zmp_to_index.argtypes = [ctypes.c_void_p, u64, ctypes.c_void_p, u64]
    return L


def build_main(directory):
    """the stand-alone program with the address and undefined-behaviour sanitizers linked in"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the members-points program"
    exe = os.path.join(str(directory), "members_points_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", exe, MAIN], check=True)
    return exe


class Found:
    def __init__(self, rc, rows, out_len, entries, stats):
        self.rc, self.rows, self.out_len, self.entries = rc, rows, out_len, entries
        self.members, self.header_candidates, self.block_candidates, self.dropped, self.rounds, self.jobs = stats

    def stats(self):
        return self.members, self.header_candidates, self.block_candidates, self.dropped, self.rounds

    def key(self):
        return (self.rc, self.rows, self.out_len, self.entries) + self.stats()


def bound(f, chunk):
    """rows a file of len(f) bytes can have: two per member of 20 bytes, one per chunk"""
    return len(f) // 10 + len(f) // chunk + 4


def h_index(H, f, chunk, spacing=1, limit=0, lanes=1, max_entries=None):
    cap = bound(f, chunk) if max_entries is None else max_entries
    buf = (u64 * (2 * max(cap, 1)))()
    entries, n = u64(0), u64(0)
    stats = (u64 * 6)()
    rc = H.zmp_index(f, len(f), chunk, spacing, limit, lanes, buf, cap, ctypes.byref(entries), ctypes.byref(n), stats)
    assert rc != -100, "the harness contradicts itself (lanes, or a walk that does not close)"
    rows = [[buf[2 * i], buf[2 * i + 1]] for i in range(entries.value)] if rc == OK else []
    return Found(rc, rows, n.value, entries.value, list(stats))


def h_candidates(H, f, chunk, lanes=1):
    """(header candidates, block candidates)"""
    hcap, bcap = len(f) // 3 + 2, len(f) // chunk + 3
    hc, bc, counts = (u64 * hcap)(), (u64 * bcap)(), (u64 * 2)()
    assert H.zmp_candidates(f, len(f), chunk, lanes, hc, hcap, bc, bcap, counts) == 0
    assert counts[0] <= hcap and counts[1] <= bcap
    return [hc[i] for i in range(counts[0])], [bc[i] for i in range(counts[1])]


def flat(rows):
    return (u64 * (2 * max(len(rows), 1)))(*[v for r in rows for v in r])


def h_to_index(H, rows):
    buf = (u64 * (2 * (len(rows) + 1)))()
    n = H.zmp_to_index(flat(rows), len(rows), buf, len(rows) + 1)
    return [[buf[2 * i], buf[2 * i + 1]] for i in range(n)]


def run_main(exe, path, chunk, limit):
    """the stand-alone program over the file `path`: (a Found, zmp_to_index's count)"""
    r = subprocess.run([exe, path, str(chunk), str(limit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.split("\n") if ln]
    head = lines[0].split()
    assert head[0] == "index" and lines[-1].split()[0] == "index_pairs"
    nums = [int(x) for x in head[1:]]
    rows = [[int(ln.split()[0], 16), int(ln.split()[1])] for ln in lines[1:-1]]
    return Found(nums[0], rows, nums[2], nums[1], nums[3:9]), int(lines[-1].split()[1])


