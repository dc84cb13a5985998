"""The device-side sidecar builder in the C ABI (include/zzflate_amd.h): zz_points_windows_device, zz_ctx_last_points_windows_stats
and zz_points_thin declared and exported, zz_points_thin's results and error codes, the argument errors of
zz_points_windows_device that need no device in the order the header gives them, and the Python mirror. What needs a live
context -- the unfinished asynchronous call, the verdicts on streams and indexes -- is in tests/test_gpu_points_windows.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64


def header():
    return open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def args_of(text, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    text = header()
    assert args_of(text, "zz_points_windows_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "const uint64_t* points", "uint64_t entries",
        "const uint64_t* fine_points", "uint64_t fine_entries", "void* d_windows", "uint32_t* d_sums", "void* d_dst", "uint64_t cap",
        "uint64_t stage_bytes", "void* hip_stream"]
    assert args_of(text, "zz_ctx_last_points_windows_stats") == ["const zz_ctx* ctx", "uint64_t* batches", "uint64_t* pending_bytes", "uint32_t* rounds"]
    assert args_of(text, "zz_points_thin") == ["const uint64_t* points", "uint64_t entries", "uint64_t spacing", "uint64_t* out",
                                               "uint64_t max_entries", "uint64_t* out_entries"]
    for name in ("zz_points_windows_device", "zz_ctx_last_points_windows_stats", "zz_points_thin"):
        assert hasattr(zz.lib, name), name


def flat(rows):
    return (u64 * (2 * len(rows)))(*[v for r in rows for v in r])


ROWS = [[0, 0], [100, 10], [200, 10], [300, 25], [400, 29], [500, 30], [600, 41], [700, 41]]


def thin(rows, spacing, cap=None, out=True):
    n = u64(77)
    cap = len(rows) if cap is None else cap
    buf = (u64 * (2 * max(cap, 1)))(*([0xEE] * (2 * max(cap, 1))))
    rc = zz.lib.zz_points_thin(flat(rows), len(rows), spacing, buf if out else None, cap, ctypes.byref(n))
    return rc, n.value, [[buf[2 * i], buf[2 * i + 1]] for i in range(min(n.value, cap))] if rc == 0 else list(buf)


def test_points_thin():
    assert thin(ROWS, 1) == (0, 8, ROWS), "spacing 1 keeps every row, the empty segments' too"
    # the first row at or behind 10, 20, 30, 40 decoded bytes; then the last row
    assert thin(ROWS, 10) == (0, 6, [[0, 0], [100, 10], [300, 25], [500, 30], [600, 41], [700, 41]])
    assert thin(ROWS, 20) == (0, 4, [[0, 0], [300, 25], [600, 41], [700, 41]])
    assert thin(ROWS, 1 << 40) == (0, 2, [[0, 0], [700, 41]])
    assert thin(ROWS[:2], 5) == (0, 2, ROWS[:2])
    # too small a buffer: the count is set, nothing is written
    rc, n, buf = thin(ROWS, 10, cap=5)
    assert (rc, n) == (zz.E_NOSPACE, 6) and buf == [0xEE] * 10
    assert thin(ROWS, 10, out=False)[:2] == (zz.E_NOSPACE, 6)
    # argument errors
    n = u64(77)
    buf = (u64 * 16)()
    L = zz.lib
    assert L.zz_points_thin(None, 8, 10, buf, 8, ctypes.byref(n)) == zz.E_ARG and n.value == 77
    assert L.zz_points_thin(flat(ROWS), 8, 10, buf, 8, None) == zz.E_ARG
    assert L.zz_points_thin(flat(ROWS), 1, 10, buf, 8, ctypes.byref(n)) == zz.E_ARG and n.value == 0
    assert L.zz_points_thin(flat(ROWS), 8, 0, buf, 8, ctypes.byref(n)) == zz.E_ARG and b"spacing" in L.zz_last_error()


def test_argument_errors_before_anything_is_launched():
    """in the header's order. None of them touches the context, so a block of zeros stands in for one here; the sidecar's arrays are
    0xEE and stay so."""
    L = zz.lib
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = src = ctypes.cast(fake, ctypes.c_void_p)
    rows = flat(ROWS)
    win = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    sums = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    W, S = ctypes.cast(win, ctypes.c_void_p), ctypes.cast(sums, ctypes.c_void_p)

    def call(c=ctx, s=src, fmt=0, p=rows, e=8, fp=None, fe=0, w=W, sm=S, dst=None, cap=0, stage=0):
        return L.zz_points_windows_device(c, s, 100, fmt, p, e, fp, fe, w, sm, dst, cap, stage, None)
    for kw in (dict(c=None), dict(s=None), dict(p=None), dict(w=None), dict(sm=None)):
        assert call(**kw) == zz.E_ARG and b"null" in L.zz_last_error(), kw
        assert call(fmt=9, e=1, stage=1 << 40, **kw) == zz.E_ARG and b"null" in L.zz_last_error(), kw
    for e in (0, 1):
        assert call(e=e, fmt=9) == zz.E_ARG and b"two rows" in L.zz_last_error()
    assert call(e=(1 << 31) + 1, fmt=9) == zz.E_ARG and b"2^31" in L.zz_last_error()
    for fmt in (3, -1, 9):
        assert call(fmt=fmt, stage=1 << 40) == zz.E_ARG and b"format" in L.zz_last_error()
    assert call(stage=(64 << 20) + 1, cap=5) == zz.E_ARG and b"stage_bytes" in L.zz_last_error()
    assert call(cap=5) == zz.E_ARG and b"null buffer" in L.zz_last_error()
    # fine_points: every row of points with the same two numbers, the same first and last row
    for fine in (ROWS[:3] + ROWS[4:], ROWS[:-1], ROWS[1:], [[0, 0], [100, 11]] + ROWS[2:], ROWS[:2]):
        assert call(fp=flat(fine), fe=len(fine)) == zz.E_ARG and b"fine_points" in L.zz_last_error(), fine
    # a destination below the last out_byte: nothing is written
    dst = ctypes.create_string_buffer(64)
    assert call(dst=ctypes.cast(dst, ctypes.c_void_p), cap=40) == zz.E_NOSPACE
    more = ROWS[:3] + [[250, 20]] + ROWS[3:]
    assert call(fp=flat(more), fe=len(more), dst=ctypes.cast(dst, ctypes.c_void_p), cap=40) == zz.E_NOSPACE, "a superset passes the walk"
    assert win.raw == b"\xEE" * 64 and sums.raw == b"\xEE" * 64
    assert L.zz_ctx_last_points_windows_stats(None, None, None, None) == zz.E_ARG


def test_python_wrappers():
    sig = inspect.signature(zz.Context.points_windows)
    assert list(sig.parameters) == ["self", "src", "src_len", "points", "format", "fine_points", "dst", "cap", "stage_bytes", "stream"]
    assert [sig.parameters[k].default for k in ("format", "fine_points", "dst", "cap", "stage_bytes", "stream")] == [zz.Format.Zlib, None, None, None, 0, None]
    sig = inspect.signature(zz.Context.open_found)
    assert list(sig.parameters) == ["self", "src", "src_len", "format", "chunk_bytes", "spacing", "dst", "cap", "stream"]
    assert [sig.parameters[k].default for k in ("format", "chunk_bytes", "spacing", "dst", "cap", "stream")] == [zz.Format.Zlib, zz.POINTS_CHUNK, zz.POINTS_SPACING, None, None, None]
    assert list(inspect.signature(zz.Context.last_points_windows_stats).parameters) == ["self"]
    assert list(inspect.signature(zz.points_thin).parameters) == ["points", "spacing"]
    rows = torch.tensor(ROWS, dtype=torch.int64)
    got = zz.points_thin(rows, 20)
    assert got.device.type == "cpu" and got.dtype == torch.int64 and got.tolist() == [[0, 0], [300, 25], [600, 41], [700, 41]]
    with pytest.raises(TypeError):
        zz.points_thin(ROWS, 20)
    with pytest.raises(TypeError):
        zz.points_thin(rows.to(torch.int32), 20)
    with pytest.raises(TypeError):
        zz.points_thin(rows, 2.0)
    with pytest.raises(TypeError):
        zz.points_thin(rows, True)
    with pytest.raises(ValueError):
        zz.points_thin(rows, 0)
    with pytest.raises(ValueError):
        zz.points_thin(rows[:1], 5)
    # Context.points_windows checks its tensors before it touches the context: no device is needed to see that
    pwin = zz.Context.points_windows
    for bad in (dict(points=ROWS), dict(points=rows.to(torch.int32)), dict(points=rows.t().contiguous()), dict(points=rows, fine_points=ROWS),
                dict(points=rows, stage_bytes=1.5), dict(points=rows, stage_bytes=True), dict(points=rows, dst=[1, 2]), dict(points=rows, cap=5)):
        with pytest.raises(TypeError):
            pwin(None, 0, 100, **bad)
    with pytest.raises(ValueError):
        pwin(None, 0, 100, rows, stage_bytes=-1)
    with pytest.raises(ValueError):
        pwin(None, 0, 100, rows[:1])
