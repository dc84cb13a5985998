"""The cases of the sidecar built on the device (zz_points_windows_device, zz_points_thin): the streams of points_cases.py and the
spacings of points_ranges_cases.py -- nothing is added to either -- with zz_points_windows_host's sidecar as the yardstick. Shared
by the CPU harness's tests (test_points_windows_cpu.py) and the device's (test_gpu_points_windows.py); also the ctypes face of
tests/cxx/points_windows_harness.cpp and the plan of a call (batches, seams, pieces) computed from the rows alone."""
import ctypes
import functools
import os
import shutil
import subprocess

import zzflate_amd as zz

import points_cases as pc
import points_ranges_cases as prc

HARNESS = os.path.join(pc.ROOT, "tests", "cxx", "points_windows_harness.cpp")
MAIN = os.path.join(pc.ROOT, "tests", "cxx", "points_windows_main.cpp")
u64 = ctypes.c_uint64
WINDOW = prc.WINDOW
BATCH = pc.BATCH                                        # ZZ_INF_BATCH_BYTES: what stage_bytes = 0 means, and the most
BATCH_SEGMENTS = 1 << 20                                # ZZ_PT_BATCH_SEGMENTS
OK, NOSPACE, ARG, UNSUPPORTED, DATA = prc.OK, prc.NOSPACE, prc.ARG, prc.UNSUPPORTED, prc.DATA
GUARD = 64

STREAMS = ("alice_l6", "alice_mem1", "alice_flushes", "alice_l0", "alice_fixed", "alice_gzip_header", "alice_raw", "mix_l6", "mix_l9_raw",
           "periodic_l6", "zeros_l6", "empty_zlib", "empty_gzip", "empty_raw", "one_zlib", "one_gzip", "one_raw")
SPACINGS = prc.SPACINGS
SMALL_STAGES = (65536, 40000)                           # 40000: a first batch below 32 KiB of the next base, bases no multiple of 32 KiB
TINY_STAGE = 4096                                       # with the spacing-1 rows of alice_mem1: batches shorter than the carry
FMT = {pc.ZLIB: zz.Format.Zlib, pc.GZIP: zz.Format.Gzip, pc.RAW: zz.Format.Deflate}


# ---- rows and the yardstick, each made once -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_of(name, spacing):
    """the point index of the case at `spacing`, by zz_points_index_host: a CPU tensor"""
    s, fmt, data = pc.case(name)
    points, n = zz.points_index_host(s, FMT[fmt], spacing)
    assert n == len(data)
    return points


@functools.lru_cache(maxsize=None)
def host_sidecar(name, spacing):
    """(windows, sums) of zz_points_windows_host for rows_of(name, spacing): CPU tensors, zeros where the format says nothing"""
    s, fmt, _ = pc.case(name)
    return zz.points_windows_host(s, rows_of(name, spacing), FMT[fmt])


def as_lists(points):
    return [[int(a), int(b)] for a, b in points.tolist()]


def longest(rows):
    return max(b[1] - a[1] for a, b in zip(rows, rows[1:]))


# ---- the plan of a call, from the rows alone ------------------------------------------------------------------------------------------
def batch_end(rows, k0, limit, last=None):
    """zi_points_batches over rows[: last + 1]: the batch that begins with segment k0 ends in front of segment (return value)"""
    n = len(rows) if last is None else last + 1
    k1 = k0 + 1
    while k1 + 1 < n and k1 - k0 < BATCH_SEGMENTS and rows[k1 + 1][1] - rows[k0][1] <= limit:
        k1 += 1
    return k1


class Plan:
    """what an honest call does: decode batches, units (what lies on the stage at once) as (base, end, cut offsets, tail offset or
    None), units but the first whose base lies below 32 KiB, slots that take bytes from carry and batch both, segments cut in pieces"""
    def __init__(self, rows, fine, stage_bytes, onto_dst=False):
        stage = stage_bytes or BATCH
        dec = fine if fine is not None else rows
        self.code = UNSUPPORTED if longest(dec) > stage else OK
        self.batches = self.low_bases = self.seams = self.pieces = self.multi = 0
        self.units = []
        if self.code != OK:
            return
        at = {tuple(r): i for i, r in enumerate(dec)}
        segments = len(rows) - 1
        k0 = 0
        while k0 < segments:
            k1 = batch_end(rows, k0, stage)
            f0, f1 = at[tuple(rows[k0])], at[tuple(rows[k1])]
            # (rows with equal numbers cannot occur: bits ascend strictly)
            self.multi += sum(1 for k in range(k0, k1) if at[tuple(rows[k + 1])] - at[tuple(rows[k])] > 1)
            tail = rows[k1][1] if k1 < segments else None
            if rows[k1][1] - rows[k0][1] <= stage:
                self._unit(dec, f0, f1, [r[1] for r in rows[k0: k1]], tail, stage, onto_dst)
            else:
                self.pieces += 1
                g0 = f0
                while g0 < f1:
                    g1 = batch_end(dec, g0, stage, f1)
                    self._unit(dec, g0, g1, [dec[g0][1]], tail if g1 == f1 else dec[g1][1], stage, onto_dst)
                    g0 = g1
            k0 = k1

    def _unit(self, dec, g0, g1, cuts, tail, stage, onto_dst):
        base, end = dec[g0][1], dec[g1][1]
        if self.units and base < WINDOW:
            self.low_bases += 1
        h0 = g0
        while h0 < g1:
            h0 = batch_end(dec, h0, stage, g1)
            self.batches += 1
        if not onto_dst:
            self.seams += sum(1 for o in cuts + ([tail] if tail is not None else []) if base > 0 and base < o < base + WINDOW)
        self.units.append((base, end, cuts, tail))


# ---- the list ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """[(stream, sidecar spacing, fine: decode with the spacing-1 rows, stage_bytes)]"""
    out = []
    for name in STREAMS:
        dense = as_lists(rows_of(name, 1))
        for spacing in SPACINGS:
            rows = as_lists(rows_of(name, spacing))
            for fine in (False, True):
                dec = dense if fine else rows
                stages = [0] + list(SMALL_STAGES) + [longest(dec)]
                if name == "alice_mem1" and fine and longest(dec) <= TINY_STAGE:
                    stages.append(TINY_STAGE)
                for stage in stages:
                    if stage not in [c[3] for c in out if c[:3] == (name, spacing, fine)]:
                        out.append((name, spacing, fine, stage))
    return tuple(out)


def case_id(c):
    return "%s-s%d-%s-stage%d" % (c[0], c[1], "fine" if c[2] else "same", c[3])


def plan_of(c, onto_dst=False):
    name, spacing, fine, stage = c
    return Plan(as_lists(rows_of(name, spacing)), as_lists(rows_of(name, 1)) if fine else None, stage, onto_dst)


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DZZ_INFLATE_CHECKED"]


def build_harness(directory):
    """built as points_cases.build_harness builds its own"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the points windows harness"
    so = os.path.join(str(directory), "libpoints_windows_harness.so")
    subprocess.run([gxx] + FLAGS + ["-fPIC", "-shared", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.zpw_build.restype = ctypes.c_int
    L.zpw_build.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, vp, u64, vp, u64, vp, vp, vp, u64, u64, ctypes.c_uint32, vp]
    L.zpw_thin.restype = ctypes.c_int
    L.zpw_thin.argtypes = [vp, u64, u64, vp, u64, ctypes.POINTER(u64)]
    L.zpw_superset.restype = ctypes.c_int
    L.zpw_superset.argtypes = [vp, u64, vp, u64]
    return L


def build_main(directory):
    """the same harness behind a main(), with -fsanitize=address,undefined: a stand-alone program, nothing is preloaded"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the points windows harness"
    exe = os.path.join(str(directory), "points_windows_main")
    subprocess.run([gxx] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, MAIN], check=True)
    return exe


class Built:
    def __init__(self, rc, windows, sums, out, stats):
        self.rc, self.windows, self.sums, self.out = rc, windows, sums, out
        self.batches, self.pending, self.rounds, self.low_bases, self.seams, self.pieces = stats[:6]


def h_build(H, s, fmt, rows, fine=None, stage=0, cap=None, lanes=1):
    """the whole call on the harness. rows, fine: lists of [in_bit, out_byte]; cap: None, or the capacity of a destination. Both
    arrays and the destination lie between GUARD bytes that must come back untouched; they start as 0xEE, so that what the call
    leaves unwritten shows."""
    segments = max(len(rows) - 1, 1)
    win = ctypes.create_string_buffer(b"\xEE" * (segments * WINDOW + 2 * GUARD), segments * WINDOW + 2 * GUARD)
    sums = ctypes.create_string_buffer(b"\xEE" * (segments * 4 + 2 * GUARD), segments * 4 + 2 * GUARD)
    dst = None if cap is None else ctypes.create_string_buffer(b"\xEE" * (cap + 2 * GUARD), cap + 2 * GUARD)
    stats = (u64 * 8)()
    rc = H.zpw_build(s, len(s), fmt, pc.flat(rows), len(rows), None if fine is None else pc.flat(fine), 0 if fine is None else len(fine),
                     ctypes.addressof(win) + GUARD, ctypes.addressof(sums) + GUARD, None if dst is None else ctypes.addressof(dst) + GUARD,
                     0 if cap is None else cap, stage, lanes, stats)
    assert rc != -100, "the harness contradicts itself (lanes, counts, pointers or sums)"
    e = b"\xEE" * GUARD
    assert win.raw[:GUARD] == e and win.raw[-GUARD:] == e and sums.raw[:GUARD] == e and sums.raw[-GUARD:] == e, "bytes outside the sidecar were written"
    out = None
    if dst is not None:
        assert dst.raw[:GUARD] == e and dst.raw[-GUARD:] == e, "bytes outside the destination were written"
        out = dst.raw[GUARD: GUARD + cap]
    return Built(rc, win.raw[GUARD: -GUARD], sums.raw[GUARD: -GUARD], out, list(stats))


def host_bytes(windows, sums):
    """zz_points_windows_host's tensors as the two byte strings h_build returns"""
    return windows.numpy().tobytes(), sums.numpy().tobytes()


def h_thin(H, rows, spacing, max_entries=None):
    n = u64(0)
    cap = len(rows) if max_entries is None else max_entries
    out = (u64 * (2 * max(cap, 1)))()
    rc = H.zpw_thin(pc.flat(rows), len(rows), spacing, out, cap, ctypes.byref(n))
    return rc, [[out[2 * i], out[2 * i + 1]] for i in range(n.value)] if rc == 0 else [], n.value


# ---- damage --------------------------------------------------------------------------------------------------------------------------------
def trailer_damaged(s, fmt):
    """copies of a zlib or gzip stream that differ from it only inside the trailer: the checksum, and for gzip ISIZE"""
    out = []
    for at in ([-1, -4] if fmt == pc.ZLIB else [-8, -5, -4, -1]):
        b = bytearray(s)
        b[at] ^= 0x10
        out.append(bytes(b))
    return out
