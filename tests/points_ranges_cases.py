"""The cases of the reads through a point index with windows (zz_points_windows_host, zz_decode_points_ranges_device): the
streams of points_cases.py -- Python's zlib wrote them all -- with the bytes that were compressed, data[first : first + m], as the
yardstick everywhere. Shared by the CPU harness's tests (test_points_ranges_cases_cpu.py) and the device's
(test_gpu_decode_points_ranges.py); also the ctypes face of tests/cxx/inflate_points_ranges_harness.cpp, so that a device test
sends every stream, index and sidecar through the bounds-checked host restatement before the device sees it."""
import ctypes
import random
import shutil
import subprocess
import os

import deflate_cases
import points_cases as pc
from range_streams import Bits

HARNESS = os.path.join(pc.ROOT, "tests", "cxx", "inflate_points_ranges_harness.cpp")
u64 = ctypes.c_uint64
WINDOW = 32768
SPACINGS = (1, 4096, 32768, 1 << 40)                    # the last is larger than every stream: one segment
STAGE = 64 << 20                                        # ZZ_MR_STAGE of the product
SMALL_STAGE = 700                                       # the harness also runs with this one: waves and big segments on small inputs
OK, NOSPACE, ARG, UNSUPPORTED, DATA = 0, -2, -4, -5, -6
NONE = (1 << 64) - 1
GUARD = 64
ADLER_FORMATS = (pc.ZLIB,)


# ---- the harness ------------------------------------------------------------------------------------------------------------------
def build_harness(directory, stage=None):
    """built as points_cases.build_harness builds its own; stage: -DZZ_MR_STAGE of this build (None: the product's)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the points ranges harness"
    so = os.path.join(str(directory), "libinflate_points_ranges_harness%s.so" % ("" if stage is None else "_%d" % stage))
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED"] +
                   ([] if stage is None else ["-DZZ_MR_STAGE=%dull" % stage]) + ["-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.zpr_stage.restype = u64
    L.zpr_stage.argtypes = []
    L.zpr_windows.restype = ctypes.c_int
    L.zpr_windows.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, vp, u64, vp, vp]
    L.zpr_fold.restype = ctypes.c_int
    L.zpr_fold.argtypes = [ctypes.c_int, vp, vp, u64, ctypes.POINTER(ctypes.c_uint32)]
    L.zpr_reads.restype = ctypes.c_int
    L.zpr_reads.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, ctypes.c_uint32,
                            ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32), vp]
    assert L.zpr_stage() == (STAGE if stage is None else stage)
    return L


def h_windows(H, s, fmt, rows):
    """(status, windows as a bytearray of segments * WINDOW bytes -- zero where the format leaves them unspecified --, sums)"""
    segments = max(len(rows) - 1, 1)
    win = (ctypes.c_uint8 * (segments * WINDOW))()
    sums = (ctypes.c_uint32 * segments)()
    rc = H.zpr_windows(s, len(s), fmt, pc.flat(rows), len(rows), win, sums)
    return rc, bytearray(win), list(sums)


class Result:
    def __init__(self, rc, lens, status, outs, segments_decoded, waves, win_copied):
        self.rc, self.lens, self.status, self.outs = rc, lens, status, outs
        self.segments_decoded, self.waves, self.win_copied = segments_decoded, waves, win_copied


def h_reads(H, s, fmt, rows, windows, sums, reads, caps=None, lanes=1):
    """the whole call on the harness; `reads` = [(first, nbytes)]; caps default to nbytes. The GUARD bytes on both sides of every
    destination must come back untouched, and so must everything behind min(m, cap) of it."""
    k = len(reads)
    caps = [n for _, n in reads] if caps is None else list(caps)
    bufs = [ctypes.create_string_buffer(b"\xEE" * (c + 2 * GUARD), c + 2 * GUARD) for c in caps]
    ptrs = (ctypes.c_void_p * max(k, 1))(*[ctypes.addressof(b) + GUARD for b in bufs])
    firsts = (u64 * max(k, 1))(*[f & NONE for f, _ in reads])
    nbytes = (u64 * max(k, 1))(*[n & NONE for _, n in reads])
    cp = (u64 * max(k, 1))(*caps)
    lens = (u64 * max(k, 1))()
    status = (ctypes.c_int32 * max(k, 1))(*([77] * max(k, 1)))
    segs, waves = u64(0), ctypes.c_uint32(0)
    nseg = max(len(rows) - 1, 1)
    copied = (u64 * nseg)()
    win = (ctypes.c_uint8 * len(windows)).from_buffer_copy(bytes(windows))
    sm = (ctypes.c_uint32 * nseg)(*[v & 0xFFFFFFFF for v in sums])
    rc = H.zpr_reads(s, len(s), fmt, pc.flat(rows), len(rows), win, sm, k, firsts, nbytes, ptrs, cp, lens, status, lanes,
                     ctypes.byref(segs), ctypes.byref(waves), copied)
    assert rc != -100, "the harness contradicts itself (lanes, or ZI_RUN_POINT's promise)"
    outs = []
    for r in range(k):
        raw = bufs[r].raw
        wrote = min(lens[r], caps[r]) if status[r] == OK else caps[r]
        assert raw[:GUARD] == b"\xEE" * GUARD and raw[GUARD + wrote:] == b"\xEE" * (len(raw) - GUARD - wrote), "bytes outside a destination were written"
        outs.append(raw[GUARD: GUARD + lens[r]] if status[r] == OK else None)
    return Result(rc, [lens[r] if status[r] == OK else None for r in range(k)], list(status)[:k], outs, segs.value, waves.value, list(copied))


# ---- the reads of a stream, all in one call -----------------------------------------------------------------------------------------
def reads_for(rows, seed=1):
    """[(first, nbytes)] over the index `rows` of a stream of L = rows[-1][1] bytes"""
    L = rows[-1][1]
    u = [r[1] for r in rows]
    nseg = len(rows) - 1
    reads = [(0, L), (0, 1), (L, 10), (L, 0), (L + 1, 1)]
    if L:
        reads.append((L - 1, 1))
    ends = sorted(set(list(range(min(3, nseg))) + list(range(max(nseg - 3, 0), nseg))))
    for k in ends:
        if 0 < u[k] < L:
            reads.append((u[k] - 1, 2))                  # across the edge in front of segment k
        reads.append((u[k], u[k + 1] - u[k]))            # the segment exactly (an empty one: an empty read)
    empty = [k for k in range(nseg) if u[k] == u[k + 1]]
    for k in empty[:2] + empty[-2:]:
        reads.append((u[k], 5))                          # starting at the offset of an empty segment
    rng = random.Random(seed * 1009 + L)
    for _ in range(32):
        reads.append((rng.randrange(max(L, 1)), rng.randint(1, 70000)))
    reads.append(reads[-7])                              # a duplicated read
    reads += [(L // 3, 5000), (L // 3 + 100, 5000)]      # two overlapping reads
    return reads


def touched(rows, first, m):
    """the segments that hold a byte of [first, first + m): non-empty ones only"""
    return [k for k in range(len(rows) - 1) if rows[k][1] < first + m and rows[k + 1][1] > first and rows[k + 1][1] > rows[k][1]]


def expect(rows, data, reads, caps=None, stage=STAGE, bad_segments=()):
    """(lens, status, bytes, the call's code, segments decoded) an honest call must give, from the rows and the data alone;
    bad_segments: segments that are not what index and sidecar say"""
    L = rows[-1][1]
    caps = [n for _, n in reads] if caps is None else caps
    lens, status, outs, decoded = [], [], [], set()
    for (first, n), cap in zip(reads, caps):
        if first > L or first + n >= 1 << 64:
            st = ARG
        else:
            m = min(n, L - first)
            st = NOSPACE if m > cap else OK
        if st == OK:
            t = touched(rows, first, m)
            decoded.update(k for k in t if rows[k + 1][1] - rows[k][1] <= stage)
            if any(k in bad_segments for k in t):
                st = DATA
            elif any(rows[k + 1][1] - rows[k][1] > stage for k in t):
                st = UNSUPPORTED
        status.append(st)
        lens.append(m if st == OK else None)
        outs.append(data[first: first + m] if st == OK else None)
    code = next((c for c in (DATA, UNSUPPORTED, ARG, NOSPACE) if c in status), OK)
    return lens, status, outs, code, len(decoded)


def waves_of(rows, reads, caps=None, stage=STAGE):
    """the waves an honest call runs: touched segments in order take their rooms on the stage one after the other (a big one takes
    none), and the segment that begins at sum S belongs to wave S // stage"""
    L = rows[-1][1]
    caps = [n for _, n in reads] if caps is None else caps
    hit = set()
    for (first, n), cap in zip(reads, caps):
        if first <= L and first + n < 1 << 64 and min(n, L - first) <= cap:
            hit.update(touched(rows, first, min(n, L - first)))
    S, waves = 0, set()
    for k in sorted(hit):
        waves.add(S // stage)
        room = rows[k + 1][1] - rows[k][1]
        S += room if room <= stage else 0
    return len(waves)


# ---- damage and lies ------------------------------------------------------------------------------------------------------------------
def valid(rows, k):
    """the bytes of slot k that the format specifies: its last min(out_byte[k], WINDOW)"""
    return min(rows[k][1], WINDOW)


def aligned_segments(rows):
    """the non-empty segments behind the first whose row is a whole byte: what zlib itself can decode from, given a dictionary"""
    return [k for k in range(1, len(rows) - 1) if rows[k][0] % 8 == 0 and rows[k + 1][1] > rows[k][1]]


def damage_reads(rows, k):
    """a read inside segment k, and reads elsewhere"""
    L = rows[-1][1]
    mid = (rows[k][1] + rows[k + 1][1]) // 2
    return [(mid, 1), (0, 1), (L - 1, 1), (0, L), (rows[k + 1][1], 100), (max(rows[k][1] - 100, 0), min(100, rows[k][1]))]


def inverted_slot(windows, rows, k):
    """a copy of the windows with every valid byte of slot k inverted"""
    w = bytearray(windows)
    for i in range((k + 1) * WINDOW - valid(rows, k), (k + 1) * WINDOW):
        w[i] ^= 0xFF
    return w


def sums_off_by_one(sums, k):
    s = list(sums)
    s[k] = (s[k] + 1) & 0xFFFFFFFF
    return s


SHAPE_LIES = ("rows_swapped", "row_past_stream", "last_row_dropped", "row_duplicated", "row0_not_zero")
SEGMENT_LIES = ("bit_plus_one", "bit_mid_block", "out_off_by_one")      # the row len(rows) // 2 lies: the segments beside it are not what it says


# streams whose indexes have at least four rows: zlib (one with empty segments), gzip, raw
LIE_CASES = ("alice_mem1", "alice_flushes", "mix_l6", "mix_l9_raw")
LIE_SPACINGS = {"alice_mem1": (1, 4096), "alice_flushes": (1,), "mix_l6": (4096,), "mix_l9_raw": (4096,)}


def lied(rows, kind, s, windows, sums):
    """(rows, windows, sums) with the lie `kind` of points_cases.lie; the honest sidecar keeps one slot and one entry per segment
    of the lied rows (a dropped row drops the last, a duplicated row doubles its own)"""
    r = pc.lie(rows, kind, len(s))
    k = len(rows) // 2
    w, sm = bytearray(windows), list(sums)
    if kind == "last_row_dropped":
        w, sm = w[:-WINDOW], sm[:-1]
    elif kind == "row_duplicated":
        w = w[: k * WINDOW] + w[k * WINDOW: (k + 1) * WINDOW] + w[k * WINDOW:]
        sm = sm[:k] + [sm[k]] + sm[k:]
    return r, w, sm


def hand_made():
    """(raw stream, rows, windows, sums, data): a 10-byte stored block, then a fixed block whose first match has distance 11 -- one
    byte in front of the stream. Slot 1 holds 0xAA in front of its 10 valid bytes: whoever reads there gets a byte, and no error."""
    import zlib
    b = Bits()
    payload = b"0123456789"
    deflate_cases.stored(b, False, payload)
    second = b.n
    f = deflate_cases.Fixed(b, True)
    f.match(3, 11)
    f.sym(256)
    end = b.n
    rows = [[0, 0], [second, 10], [end, 13]]
    windows = bytearray(2 * WINDOW)
    windows[WINDOW: 2 * WINDOW - 10] = b"\xAA" * (WINDOW - 10)
    windows[2 * WINDOW - 10:] = payload
    data = payload + b"\xAA01"                            # what a decoder that trusted the slot would return
    sums = [zlib.crc32(payload), zlib.crc32(data[10:])]
    return b.bytes(), rows, windows, sums, data
