"""The device-side index builder in the C ABI (include/zzflate_amd.h): zz_points_index_bound, zz_points_index_device,
zz_ctx_last_points_index_stats and ZZ_POINTS_CHUNK_DEFAULT declared and exported, the argument errors that need no device in the
order the header gives them, zz_points_index_bound's values, and the Python mirror. What needs a live context -- the unfinished
asynchronous call, ZZ_E_NOSPACE with *entries set and nothing written -- is in tests/test_gpu_points_index.py."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64


def header():
    return open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def test_symbols_are_declared_and_exported():
    text = header()
    m = re.search(r"int\s+zz_points_index_device\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "uint64_t chunk_bytes", "uint64_t spacing",
                    "uint64_t* points", "uint64_t max_entries", "uint64_t* entries", "uint64_t* out_len", "void* hip_stream"], args
    assert re.search(r"uint64_t\s+zz_points_index_bound\s*\(\s*uint64_t src_len,\s*uint64_t chunk_bytes\s*\);", text)
    assert re.search(r"int\s+zz_ctx_last_points_index_stats\s*\(\s*const zz_ctx\* ctx,\s*uint64_t\* candidates,\s*uint64_t\* dropped,\s*uint32_t\* rounds\s*\);", text)
    assert re.search(r"#define ZZ_POINTS_CHUNK_DEFAULT 16384ull", text)
    for name in ("zz_points_index_device", "zz_points_index_bound", "zz_ctx_last_points_index_stats"):
        assert hasattr(zz.lib, name), name
    assert zz.POINTS_CHUNK == 16384
    assert "NOT" in text[text.index("The point index built ON THE DEVICE"): text.index("#define ZZ_POINTS_CHUNK_DEFAULT")], \
        "the header says that ZZ_OK is no verdict on the stream"


def test_bound():
    B = zz.lib.zz_points_index_bound
    assert [B(n, 16384) for n in (0, 1, 16384, 16385, 1 << 30)] == [2, 2, 2, 3, 65537]       # chunks + 1; an empty stream has one chunk
    assert B(1000, 16) == 64 and B(1001, 16) == 64 and B(1009, 16) == 65
    assert B(1000, 15) == 0 and B(1000, 0) == 0, "chunk_bytes below 16: no bound"
    assert zz.points_index_bound(100000) == 8 and zz.points_index_bound(100000, 1000) == 101


def test_argument_errors_before_anything_is_launched():
    """in the header's order: null pointers; chunk_bytes and spacing; the format. None of them touches the context, so a block of
    zeros stands in for one here."""
    L = zz.lib
    fake = ctypes.create_string_buffer(1 << 16)
    ctx, src = ctypes.cast(fake, ctypes.c_void_p), ctypes.cast(fake, ctypes.c_void_p)
    rows = (u64 * 8)(*([0xEE] * 8))
    e, n = u64(7), u64(7)
    call = lambda c, s, fmt, chunk, spacing, pe, pn: L.zz_points_index_device(c, s, 100, fmt, chunk, spacing, rows, 4, pe, pn, None)
    E, N = ctypes.byref(e), ctypes.byref(n)
    # null context, source, entries, out_len -- each alone, and with every later error present too
    for bad in ((None, src, E, N), (ctx, None, E, N), (ctx, src, None, N), (ctx, src, E, None)):
        for fmt, chunk, spacing in ((0, 16384, 1), (9, 15, 0)):
            assert call(bad[0], bad[1], fmt, chunk, spacing, bad[2], bad[3]) == zz.E_ARG
            assert b"null" in L.zz_last_error()
    assert (e.value, n.value) == (7, 7), "nothing is written before the null checks have passed"
    # chunk_bytes < 16, then spacing < 1 -- in front of the format
    assert call(ctx, src, 9, 15, 0, E, N) == zz.E_ARG and b"chunk_bytes" in L.zz_last_error()
    assert (e.value, n.value) == (0, 0)
    assert call(ctx, src, 9, 0, 1, E, N) == zz.E_ARG and b"chunk_bytes" in L.zz_last_error()
    assert call(ctx, src, 9, 16, 0, E, N) == zz.E_ARG and b"spacing" in L.zz_last_error()
    # a format outside 0..2
    for fmt in (3, -1, 9):
        assert call(ctx, src, fmt, 16, 1, E, N) == zz.E_ARG and b"format" in L.zz_last_error()
    assert list(rows) == [0xEE] * 8
    assert L.zz_ctx_last_points_index_stats(None, None, None, None) == zz.E_ARG


def test_python_wrappers():
    sig = inspect.signature(zz.Context.points_index)
    assert list(sig.parameters) == ["self", "src", "src_len", "format", "chunk_bytes", "spacing", "stream"]
    assert (sig.parameters["format"].default, sig.parameters["chunk_bytes"].default, sig.parameters["spacing"].default,
            sig.parameters["stream"].default) == (zz.Format.Zlib, zz.POINTS_CHUNK, 1, None)
    sig = inspect.signature(zz.Context.decode_found)
    assert list(sig.parameters) == ["self", "src", "src_len", "dst", "cap", "format", "chunk_bytes", "stream"]
    assert sig.parameters["chunk_bytes"].default == zz.POINTS_CHUNK
    assert list(inspect.signature(zz.Context.last_points_index_stats).parameters) == ["self"]
    assert list(inspect.signature(zz.points_index_bound).parameters) == ["src_len", "chunk_bytes"]
