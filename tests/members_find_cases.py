"""The cases of the members found in parallel (zz_members_find_device, zz_decode_members_found_device): member files written with
Python's zlib / gzip (through members_cases' builders), the pure-Python restatement of the definition -- candidates by the header
rule, the true chain from ``decompressobj(31).unused_data`` -- and the yardstick, zlib's member loop (members_cases.yardstick).
Shared by the CPU harness's tests (test_members_find_cpu.py) and the device's (test_gpu_members_find.py); also the ctypes face of
tests/cxx/members_find_harness.cpp and the build of the stand-alone program tests/cxx/members_find_main.cpp."""
import ctypes
import functools
import gzip
import os
import random
import shutil
import struct
import subprocess
import zlib

import members_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cxx", "members_find_harness.cpp")
MAIN = os.path.join(ROOT, "tests", "cxx", "members_find_main.cpp")
u64 = ctypes.c_uint64

OK, NOSPACE, UNSUPPORTED, DATA = 0, -2, -5, -6
LIMIT_DEFAULT = 1 << 20                                         # ZZ_MEMBERS_FIND_LIMIT_DEFAULT
LIMITS = (64, 4096, LIMIT_DEFAULT)
STRETCH = mc.STRETCH                                            # source bytes per workgroup of the mark pass
PER_LANE = 16                                                   # and per lane
ISIZE_MAGIC = 0x00088B1F                                        # 559,903: an ISIZE whose bytes are 1f 8b 08 00


# ---- the definition, restated -------------------------------------------------------------------------------------------------------
def header_len(f, i):
    """zi_header for gzip at f[i:]: the header's length, or -1"""
    h = f[i:]
    if len(h) < 10 or h[:3] != b"\x1f\x8b\x08" or h[3] & 0xE0:
        return -1
    flg, p = h[3], 10
    if flg & 4:
        if p + 2 > len(h):
            return -1
        p += 2 + struct.unpack_from("<H", h, p)[0]
        if p > len(h):
            return -1
    for bit in (8, 16):
        if flg & bit:
            z = h.find(b"\x00", p)
            if z < 0:
                return -1
            p = z + 1
    if flg & 2:
        if p + 2 > len(h) or zlib.crc32(h[:p]) & 0xFFFF != struct.unpack_from("<H", h, p)[0]:
            return -1
        p += 2
    return p


def candidates(f):
    """offset 0, and every offset i >= 20 with a header that leaves ten bytes behind it"""
    out, at = ([0] if f else []), f.find(b"\x1f\x8b\x08", 20)
    while at >= 0:
        hl = header_len(f, at)
        if hl >= 0 and at + hl + 10 <= len(f):
            out.append(at)
        at = f.find(b"\x1f\x8b\x08", at + 1)
    return out


def true_chain(f):
    """[(file offset, decoded offset)] of every member and the last row (len(f), L), from zlib's own member loop; the members'
    lengths in the file (header, blocks, trailer) beside it. The file must be valid."""
    rows, used, pos, off, rest = [], [], 0, 0, f
    while rest:
        d = zlib.decompressobj(31)
        o = d.decompress(rest)
        assert d.eof, "the file is meant to be valid"
        rows.append([pos, off]); used.append(len(rest) - len(d.unused_data))
        pos += used[-1]; off += len(o)
        rest = d.unused_data
    return rows + [[len(f), off]], used


class Expect:
    """what the definition gives for a valid file"""

    def __init__(self, f, stored_long=False):
        self.rows, self.used = true_chain(f)
        self.members = len(self.rows) - 1
        self.cand = candidates(f)
        assert all(r[0] in self.cand for r in self.rows[:-1]), "every true member start is a candidate"
        self.dropped = len(self.cand) - self.members
        self.stored_long = stored_long

    def rounds(self, limit):
        """1 if no member behind the first passes the limit, 2 if one passes it by more than its last symbols (three bytes), else
        None: the member ends within a symbol of the limit, or holds stored blocks, which are not given up inside"""
        over = [u - 8 - limit for u in self.used[1:]]
        if all(o <= 0 for o in over):
            return 1
        if self.stored_long or any(0 < o <= 3 for o in over):
            return None
        return 2


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def sized(size, rng):
    """a plain member (no `BC`) of exactly `size` bytes: eight stored random bytes and a filler subfield"""
    data = bytes(rng.getrandbits(8) for _ in range(8))
    base = len(mc.member(data, 0, extra=mc.subfield(b"ZZ", b"")))
    assert size >= base
    m = mc.member(data, 0, extra=mc.subfield(b"ZZ", b"\x00" * (size - base)))
    assert len(m) == size
    return m, data


def stored_with(payload):
    """a level-0 member whose stored blocks hold `payload` verbatim"""
    m = mc.member(payload, 0)
    assert payload[:60000] in m
    return m


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: (file, stored_long)} -- every file is valid; stored_long: a member behind the first is longer than a small limit and holds
    stored blocks (see Expect.rounds)"""
    rng = random.Random(22)
    alice, fields, cp = mc.corpus("alice29.txt"), mc.corpus("fields.c"), mc.corpus("cp.html")
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), fields[:5000]
    cases = {}
    cases["three corpus members at levels 1, 6 and 9"] = (mc.member(alice[:70000], 1) + mc.member(fields, 6) + mc.member(cp, 9), False)
    cases["python gzip.compress members"] = (gzip.compress(a) + gzip.compress(b, 1) + gzip.compress(c, 9), False)
    cases["one member"] = (mc.member(a), False)
    cases["FNAME, FCOMMENT, FHCRC and a non-BC FEXTRA"] = (
        mc.member(a, name=b"a.txt") + mc.member(b, comment=b"the second") + mc.member(c, hcrc=True)
        + mc.member(a, extra=mc.subfield(b"AB", b"hello") + mc.subfield(b"XY", b"")) + mc.member(b, extra=b"", name=b"n", comment=b"c", hcrc=True), False)
    tiny = [mc.text(rng.randrange(201), k) if k % 7 else b"" for k in range(2000)]
    cases["2,000 members of 0..200 bytes"] = (b"".join(mc.member(t, (1, 6, 9, 0)[k & 3]) for k, t in enumerate(tiny)), False)
    cases["BGZF and plain members mixed"] = (mc.bgzf(a) + mc.member(b) + mc.bgzf(c) + gzip.compress(a) + mc.EOF_BLOCK + mc.member(b"") + mc.bgzf(b), False)
    for at in (STRETCH - 1, STRETCH, STRETCH + 1):
        cases[f"a member start at file offset {at}"] = (sized(at, rng)[0] + mc.member(b) + mc.member(a, 1), False)
    parts, pos = [], 0
    for k, past in enumerate((PER_LANE - 1, PER_LANE, PER_LANE + 1)):
        parts.append(sized((k + 1) * STRETCH + past - pos, rng)[0]); pos = (k + 1) * STRETCH + past
        parts.append(mc.member(mc.text(700, k))); pos += len(parts[-1])
    cases["member starts 15, 16 and 17 past a stretch start"] = (b"".join(parts), False)
    junk = bytes(rng.getrandbits(8) | 1 for _ in range(300))
    inner = mc.member(mc.text(800, 9), 6, name=b"inner")
    payload = junk[:100] + b"\x1f\x8b\x08\x00" + junk[100:200] + inner + junk[200:] + b"\x1f\x8b\x08\x00\x00\x00"
    cases["stored bytes that look like headers and like a member"] = (mc.member(a) + mc.member(b, 1) + stored_with(payload), False)
    cases["stored look-alikes in the first member"] = (stored_with(payload[:-6]) + mc.member(a), False)
    big = mc.text(ISIZE_MAGIC, 3)
    cases["ISIZE 1f 8b 08 00 in front of the next member"] = (mc.member(big, 6) + mc.member(a) + mc.member(b), False)
    cases["a member many times longer than a small limit"] = (mc.member(a) + mc.member(alice[:100000], 6) + mc.member(c), False)
    cases["a long stored member behind the first"] = (mc.member(a) + mc.member(bytes(rng.getrandbits(8) for _ in range(70000)), 0) + mc.member(c), True)
    return cases


def small_three():
    """a three-member file of about 150 bytes for the sweeps"""
    ms = [mc.member(b"first member, "), mc.member(b"the second one is a little longer than the first, ", name=b"2"), mc.member(b"and the third.", 1)]
    return b"".join(ms), ms


@functools.lru_cache(maxsize=None)
def refusal_cases():
    """{name: file}: zlib refuses every one of them"""
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), mc.corpus("fields.c")[:5000]
    ms = [mc.member(a), mc.member(b, 1), mc.member(c, 9)]
    good = b"".join(ms)
    starts = [0, len(ms[0]), len(ms[0]) + len(ms[1])]
    cases = {"the empty file": b""}
    for name, byte in (("a zero byte", b"\x00"), ("a junk byte", b"\x5a")):
        cases[name + " between members"] = ms[0] + byte + ms[1] + ms[2]
        cases[name + " behind the last member"] = good + byte

    def flipped(pos, bit=0):
        f = bytearray(good); f[pos] ^= 1 << bit
        return bytes(f)
    for k, nm in enumerate(("the first", "the middle", "the last")):
        end = starts[k] + len(ms[k])
        cases[f"a flipped bit in the header of {nm} member"] = flipped(starts[k] + 2)
        cases[f"a flipped bit in the blocks of {nm} member"] = flipped(starts[k] + 10 + 200, 3)
        cases[f"a flipped bit in the CRC of {nm} member"] = flipped(end - 8)
        cases[f"a flipped bit in the ISIZE of {nm} member"] = flipped(end - 4)
    f, three = small_three()
    ends = (len(three[0]), len(three[0]) + len(three[1]))             # (a cut behind a whole member leaves a valid file)
    for cut in range(1, len(f)):
        if cut not in ends:
            cases[f"three small members cut to {cut} bytes"] = f[:cut]
    for name, s in cases.items():
        assert mc.yardstick(s) is None, name
    return cases


def crc_damaged():
    """(file, the undamaged file, the damaged member): a flipped CRC bit in member 0, members 1 and 2 whole"""
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), mc.corpus("fields.c")[:5000]
    ms = [mc.member(a), mc.member(b, 1), mc.member(c, 9)]
    good = b"".join(ms)
    f = bytearray(good); f[len(ms[0]) - 8] ^= 1
    return bytes(f), good, 0


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def build_harness(directory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the members-find harness"
    so = os.path.join(str(directory), "libmembers_find_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    L.zmf_find.restype = ctypes.c_int
    L.zmf_find.argtypes = [ctypes.c_char_p, u64, u64, ctypes.c_uint32, ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.c_void_p]
    L.zmf_decode.restype = ctypes.c_int
    L.zmf_decode.argtypes = [ctypes.c_char_p, u64, ctypes.c_void_p, u64, u64, ctypes.c_uint32, ctypes.POINTER(u64), ctypes.c_void_p]
    L.zmf_candidates.restype = ctypes.c_int64
    L.zmf_candidates.argtypes = [ctypes.c_char_p, u64, ctypes.c_void_p, u64]
    return L


def build_main(directory):
    """the stand-alone program with the address and undefined-behaviour sanitizers linked in"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the members-find program"
    exe = os.path.join(str(directory), "members_find_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", exe, MAIN], check=True)
    return exe


class Found:
    def __init__(self, rc, rows, entries, stats):
        self.rc, self.rows, self.entries = rc, rows, entries
        self.members, self.candidates, self.dropped, self.rounds, self.jobs = stats

    def key(self):
        return self.rc, self.rows, self.entries, self.members, self.candidates, self.dropped, self.rounds


def h_find(H, f, limit=LIMIT_DEFAULT, lanes=1, max_entries=None):
    cap = len(f) // 20 + 2 if max_entries is None else max_entries
    buf = (u64 * (2 * max(cap, 1)))()
    entries = u64(0)
    stats = (u64 * 5)()
    rc = H.zmf_find(f, len(f), limit, lanes, buf, cap, ctypes.byref(entries), stats)
    assert rc != -100, "the harness contradicts itself"
    rows = [[buf[2 * i], buf[2 * i + 1]] for i in range(entries.value)] if rc == OK else []
    return Found(rc, rows, entries.value, list(stats))


def h_decode(H, f, cap, limit=LIMIT_DEFAULT, lanes=1):
    """(status, decoded bytes or None, stats)"""
    out = ctypes.create_string_buffer(cap + 1)
    n = u64(0)
    stats = (u64 * 5)()
    rc = H.zmf_decode(f, len(f), out, cap, limit, lanes, ctypes.byref(n), stats)
    assert rc != -100, "the harness contradicts itself"
    return rc, (out.raw[:n.value] if rc == OK else None), list(stats)


def h_candidates(H, f):
    cap = len(f) // 3 + 2
    buf = (u64 * cap)()
    n = H.zmf_candidates(f, len(f), buf, cap)
    assert 0 <= n <= cap
    return [buf[i] for i in range(n)]


def run_main(exe, path, limit, cap):
    """the stand-alone program over the file `path`: (a Found, (decode status, out_len, crc32))"""
    r = subprocess.run([exe, path, str(limit), str(cap)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.split("\n") if ln]
    head = lines[0].split()
    assert head[0] == "find" and lines[-1].split()[0] == "decode"
    nums = [int(x) for x in head[1:]]
    rows = [[int(x) for x in ln.split()] for ln in lines[1:-1]]
    return Found(nums[0], rows, nums[1], nums[2:7]), tuple(int(x) for x in lines[-1].split()[1:])


def verdict(want, cap):
    """(status, bytes) the yardstick sets for a decode into `cap` bytes of room -- for files whose first failing member, if any, is
    refused before its bytes pass the room (every refusal of refusal_cases decoded with room for the whole file)"""
    if want is None:
        return DATA, None
    return (OK, want) if len(want) <= cap else (NOSPACE, None)
