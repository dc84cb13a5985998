"""The reads through a point index with windows in the C ABI (include/zzflate_amd.h): the three entry points are declared with
the documented signatures and exported, every before-launch argument error is refused without a device, the builder's argument
errors and verdicts come without one too, and the Python wrappers check types, shapes and devices before anything is called."""
import ctypes
import inspect
import os
import re
import types
import zlib

import pytest
import torch

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64


def declared(name):
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    assert declared("zz_points_windows_host") == [
        "const uint8_t* src", "uint64_t src_len", "int format", "const uint64_t* points", "uint64_t entries", "uint8_t* windows",
        "uint32_t* sums"]
    assert declared("zz_decode_points_ranges_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "const uint64_t* d_points", "uint64_t entries",
        "const void* d_windows", "const uint32_t* d_sums", "uint64_t nranges", "const uint64_t* d_firsts", "const uint64_t* d_nbytes",
        "void* const* d_dsts", "const uint64_t* d_caps", "uint64_t* d_out_lens", "int32_t* d_status", "void* hip_stream"]
    assert declared("zz_ctx_last_decode_points_ranges_stats") == ["const zz_ctx* ctx", "uint64_t* segments_decoded", "uint32_t* waves"]
    for name in ("zz_points_windows_host", "zz_decode_points_ranges_device", "zz_ctx_last_decode_points_ranges_stats"):
        assert hasattr(zz.lib, name), name
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    assert re.search(r"#define ZZ_POINTS_WINDOW 32768u", text) and zz.POINTS_WINDOW == 32768
    assert re.search(r"#define ZZ_POINTS_SPACING_DEFAULT 131072ull", text)         # left alone
    doc = text[text.index("windows and sums beside the index"): text.index("int zz_points_windows_host")]
    assert "3.1 %" in doc and "25 %" in doc and "grows with the spacing" in doc    # the header states the trade
    doc = text[text.index("Many reads of one zlib / gzip / raw stream"): text.index("int zz_decode_points_ranges_device")]
    assert "NOTHING BESIDE THE STREAM IS TRUSTED" in doc and "Workspace" in doc


def call(ctx, src, idx, win, sums, firsts, nbytes, dsts, caps, lens, entries=5, nranges=3, status=None, fmt=0):
    return zz.lib.zz_decode_points_ranges_device(ctx, src, 100, fmt, idx, entries, win, sums, nranges, firsts, nbytes, dsts, caps, lens, status, None)


def test_argument_errors_are_refused_without_a_device():
    """none of these reaches the context: a word of host memory stands in for it"""
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    E = zz.E_ARG
    args = [p] * 10
    for i in range(10):
        a = list(args)
        a[i] = None
        assert call(*a) == E and b"null" in zz.lib.zz_last_error(), i
    assert call(*args, entries=0) == E and call(*args, entries=1) == E
    assert b"at least two rows" in zz.lib.zz_last_error()
    assert call(*args, entries=(1 << 31) + 1) == E and call(*args, entries=(1 << 64) - 1) == E
    assert b"segments" in zz.lib.zz_last_error()
    assert call(*args, nranges=1 << 31) == E and call(*args, nranges=(1 << 64) - 1) == E
    assert call(*args, fmt=3) == E and call(*args, fmt=-1) == E
    assert b"format" in zz.lib.zz_last_error()
    assert list(word) == [0] * 8


def test_no_reads_is_ok_at_once():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    args = [p] * 10
    assert call(*args, nranges=0) == 0 and call(*args, nranges=0, status=p) == 0
    assert call(*args, nranges=0, entries=1 << 31) == 0                            # 2^31 - 1 segments are the most an index holds
    assert call(*args, nranges=0, entries=1) == zz.E_ARG and call(*args, nranges=0, fmt=3) == zz.E_ARG      # the arguments are checked first
    assert list(word) == [0] * 8


def test_stats_need_a_context():
    assert zz.lib.zz_ctx_last_decode_points_ranges_stats(None, None, None) == zz.E_ARG


def test_the_builder_refuses_its_arguments_and_judges_without_a_device():
    data = b"a windows pass needs no device " * 3000
    s = zlib.compress(data, 6)
    points, n = zz.points_index_host(s, zz.Format.Zlib, 1)
    assert n == len(data)
    rows = (u64 * (2 * points.shape[0]))(*[int(v) & ((1 << 64) - 1) for v in points.flatten().tolist()])
    seg = points.shape[0] - 1
    win, sums = (ctypes.c_uint8 * (seg * 32768))(), (ctypes.c_uint32 * seg)()
    f = zz.lib.zz_points_windows_host
    assert f(s, len(s), 0, rows, seg + 1, win, sums) == 0
    assert sums[0] == zlib.adler32(data[: points[1, 1]])
    E = zz.E_ARG
    assert f(None, len(s), 0, rows, seg + 1, win, sums) == E and f(s, len(s), 0, None, seg + 1, win, sums) == E
    assert f(s, len(s), 0, rows, seg + 1, None, sums) == E and f(s, len(s), 0, rows, seg + 1, win, None) == E
    assert b"null" in zz.lib.zz_last_error()
    assert f(s, len(s), 0, rows, 1, win, sums) == E and f(s, len(s), 0, rows, 0, win, sums) == E
    assert f(s, len(s), 3, rows, seg + 1, win, sums) == E and f(s, len(s), -1, rows, seg + 1, win, sums) == E
    assert f(s, len(s), 1, rows, seg + 1, win, sums) == zz.E_DATA                  # not a gzip stream
    dict_stream = bytes([0x78, 0xBB]) + s[2:]                                      # FDICT set, FCHECK made right
    assert (0x78 * 256 + 0xBB) % 31 == 0
    assert f(dict_stream, len(s), 0, rows, seg + 1, win, sums) == zz.E_UNSUPPORTED
    # the Python face: tensors of the stated shapes; a lying index raises E_DATA
    w, sm = zz.points_windows_host(s, points, zz.Format.Zlib)
    assert w.dtype == torch.uint8 and tuple(w.shape) == (seg, 32768) and sm.dtype == torch.int32 and tuple(sm.shape) == (seg,)
    assert [v & 0xFFFFFFFF for v in sm.tolist()] == list(sums) and bytes(w.flatten().tolist()) == bytes(win)
    if seg >= 2:
        lie = points.clone()
        lie[1, 0] += 1
        with pytest.raises(zz.ZzFlateError) as e:
            zz.points_windows_host(s, lie, zz.Format.Zlib)
        assert e.value.code == zz.E_DATA
    with pytest.raises(TypeError):
        zz.points_windows_host(s, points.to(torch.int32), zz.Format.Zlib)
    with pytest.raises(TypeError):
        zz.points_windows_host(s, points.flatten(), zz.Format.Zlib)
    with pytest.raises(ValueError):
        zz.points_windows_host(s, points[:1], zz.Format.Zlib)


def test_python_interface():
    sig = inspect.signature(zz.Context.decode_points_ranges)
    assert list(sig.parameters) == ["self", "src", "src_len", "points", "windows", "sums", "firsts", "nbytes", "dsts", "caps", "format", "stream"]
    assert sig.parameters["caps"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(zz.Context.decode_points_range)
    assert list(sig.parameters) == ["self", "src", "src_len", "points", "windows", "sums", "first", "nbytes", "dst", "cap", "format", "stream"]
    assert list(inspect.signature(zz.Context.last_decode_points_ranges_stats).parameters) == ["self"]
    assert list(inspect.signature(zz.points_windows_host).parameters) == ["data", "points", "format"]


def test_python_type_shape_and_device_errors_come_before_any_call():
    """a stand-in for the context: the checks need only its device number"""
    me = types.SimpleNamespace(device=0)
    f = zz.Context.decode_points_ranges
    points = torch.zeros((3, 2), dtype=torch.int64)
    windows = torch.zeros((2, 32768), dtype=torch.uint8)
    sums = torch.zeros(2, dtype=torch.int32)
    for bad in (points.to(torch.int32), points.flatten(), torch.zeros((3, 3), dtype=torch.int64), [[0, 0], [1, 1]]):
        with pytest.raises(TypeError):
            f(me, None, 0, bad, windows, sums, [0], [1], [None])
    with pytest.raises(ValueError):
        f(me, None, 0, points[:1], windows, sums, [0], [1], [None])
    for bad in (windows.to(torch.int8), windows[:1], torch.zeros((2, 32767), dtype=torch.uint8), windows.flatten()):
        with pytest.raises(TypeError):
            f(me, None, 0, points, bad, sums, [0], [1], [None])
    for bad in (sums.to(torch.int64), sums[:1], torch.zeros((2, 1), dtype=torch.int32)):
        with pytest.raises(TypeError):
            f(me, None, 0, points, windows, bad, [0], [1], [None])
    with pytest.raises(ValueError, match="points must live on this context's device"):
        f(me, None, 0, points, windows, sums, [0], [1], [None])


def test_the_neighbours_are_what_they_were():
    assert declared("zz_points_index_host") == [
        "const uint8_t* src", "uint64_t src_len", "int format", "uint64_t spacing", "uint64_t* points", "uint64_t max_entries",
        "uint64_t* entries", "uint64_t* out_len"]
    assert declared("zz_decode_points_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "void* d_dst", "uint64_t cap", "uint64_t* out_len", "int format",
        "const uint64_t* points", "uint64_t entries", "void* hip_stream"]
    assert declared("zz_decode_members_ranges_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "const uint64_t* d_index", "uint64_t entries", "uint64_t nranges",
        "const uint64_t* d_firsts", "const uint64_t* d_nbytes", "void* const* d_dsts", "const uint64_t* d_caps", "uint64_t* d_out_lens",
        "int32_t* d_status", "void* hip_stream"]
