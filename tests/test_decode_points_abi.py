"""The point-index entry points of the C ABI (include/zzflate_amd.h): declared, exported, refused without a device where they
can be, and mirrored in Python (zz.points_index_host, Context.decode_points). The builder needs no device at all, so its
argument errors are all checked here; zz_decode_points_device's behind a live context are in tests/test_gpu_decode_points.py."""
import ctypes
import inspect
import os
import re
import zlib

import pytest

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64


def header():
    return open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def test_symbols_are_declared_and_exported():
    text = header()
    m = re.search(r"int\s+zz_decode_points_device\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0].startswith("zz_ctx*") and args[-1].startswith("void* hip_stream"), args
    assert args[6] == "int format" and args[7] == "const uint64_t* points" and args[8] == "uint64_t entries", args
    m = re.search(r"int\s+zz_points_index_host\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const uint8_t* src", "uint64_t src_len", "int format", "uint64_t spacing", "uint64_t* points", "uint64_t max_entries",
                    "uint64_t* entries", "uint64_t* out_len"], args
    assert hasattr(zz.lib, "zz_decode_points_device") and hasattr(zz.lib, "zz_points_index_host")


def test_enum_and_constants():
    text = header()
    assert re.search(r"ZZ_DECODE_SERIAL = 3, ZZ_DECODE_POINTS = 4\b", text)
    assert re.search(r"#define ZZ_POINTS_SPACING_DEFAULT 131072ull", text)
    assert zz.DECODE_POINTS == 4 and (zz.DECODE_INDEXED, zz.DECODE_DISCOVERED, zz.DECODE_SERIAL) == (1, 2, 3)
    assert zz.POINTS_SPACING == 131072


def test_decode_points_refuses_a_null_context_without_a_device():
    L = zz.lib
    rows = (u64 * 4)(0, 0, 80, 10)
    p = ctypes.cast(rows, ctypes.c_void_p)
    out = u64(7)
    assert L.zz_decode_points_device(None, None, 0, None, 0, None, 0, None, 0, None) == zz.E_ARG
    assert L.zz_decode_points_device(None, p, 10, p, 10, ctypes.byref(out), 0, p, 2, None) == zz.E_ARG
    assert L.zz_decode_points_device(None, p, 10, p, 10, ctypes.byref(out), 9, p, 1, None) == zz.E_ARG
    assert b"null" in L.zz_last_error()


def test_the_builders_argument_errors():
    L = zz.lib
    s = zlib.compress(b"abc" * 100)
    rows = (u64 * 8)()
    e, n = u64(7), u64(7)
    ok = lambda *a: L.zz_points_index_host(*a)
    assert ok(s, len(s), 0, 4096, rows, 4, ctypes.byref(e), ctypes.byref(n)) == 0 and (e.value, n.value) == (2, 300)
    assert (rows[0], rows[1], rows[3]) == (0, 0, 300) and 8 * (len(s) - 7) < rows[2] <= 8 * (len(s) - 6)    # (2 bytes of header, 4 of trailer)
    assert ok(s, len(s), 0, 4096, rows, 4, None, ctypes.byref(n)) == zz.E_ARG
    assert ok(s, len(s), 0, 4096, rows, 4, ctypes.byref(e), None) == zz.E_ARG
    assert ok(None, len(s), 0, 4096, rows, 4, ctypes.byref(e), ctypes.byref(n)) == zz.E_ARG
    assert ok(s, len(s), 3, 4096, rows, 4, ctypes.byref(e), ctypes.byref(n)) == zz.E_ARG
    assert ok(s, len(s), -1, 4096, rows, 4, ctypes.byref(e), ctypes.byref(n)) == zz.E_ARG
    assert ok(s, len(s), 0, 0, rows, 4, ctypes.byref(e), ctypes.byref(n)) == zz.E_ARG
    # a null rows pointer asks for the count: ZZ_E_NOSPACE with *entries set
    assert ok(s, len(s), 0, 4096, None, 0, ctypes.byref(e), ctypes.byref(n)) == zz.E_NOSPACE and (e.value, n.value) == (2, 300)
    # a null source of no bytes is an empty stream: invalid, not a bad argument
    assert ok(None, 0, 0, 4096, rows, 4, ctypes.byref(e), ctypes.byref(n)) == zz.E_DATA


def test_python_wrappers():
    import torch
    sig = inspect.signature(zz.points_index_host)
    assert list(sig.parameters) == ["data", "format", "spacing"]
    assert sig.parameters["format"].default == zz.Format.Zlib and sig.parameters["spacing"].default == zz.POINTS_SPACING
    sig = inspect.signature(zz.Context.decode_points)
    assert list(sig.parameters) == ["self", "src", "src_len", "dst", "cap", "points", "format", "stream"]
    assert sig.parameters["format"].default == zz.Format.Zlib and sig.parameters["stream"].default is None
    data = bytes(range(256)) * 40
    points, n = zz.points_index_host(zlib.compress(data))
    assert n == len(data) and points.dtype == torch.int64 and points.device.type == "cpu" and tuple(points.shape) == (2, 2)
    assert points[0].tolist() == [0, 0] and points[1, 1].item() == len(data)
    for bad in (4096.0, "4096", None, True):
        with pytest.raises(TypeError):
            zz.points_index_host(zlib.compress(data), zz.Format.Zlib, bad)
    with pytest.raises(ValueError):
        zz.points_index_host(zlib.compress(data), zz.Format.Zlib, 0)
    # decode_points judges `points` before it touches the device: no context is needed to see that
    ctx = object.__new__(zz.Context)
    for bad in (None, [[0, 0], [8, 1]], points.to(torch.int32), points.flatten(), points.t(), torch.zeros((2, 3), dtype=torch.int64)):
        with pytest.raises(TypeError):
            zz.Context.decode_points(ctx, 0, 0, 0, 0, bad)
