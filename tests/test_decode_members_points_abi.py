"""The decode through a member point index in the C ABI (include/zzflate_amd.h): zz_decode_members_points_device and its stats
call declared and exported, every argument error that needs no device -- zz_decode_members_found_device's rules, null points with
entries > 0, entries == 1, batch_bytes above 64 MiB -- and the Python mirror with its type errors. What needs a device is in
tests/test_gpu_decode_members_points.py."""
import ctypes
import inspect
import os
import re

import pytest

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64
ERR = (1 << 64) - 1


def header():
    return open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def args_of(text, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    text = header()
    assert args_of(text, "zz_decode_members_points_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "void* d_dst", "uint64_t cap", "uint64_t* out_len", "const uint64_t* points",
        "uint64_t entries", "uint64_t batch_bytes", "void* hip_stream"]
    assert args_of(text, "zz_ctx_last_decode_members_points_stats") == [
        "const zz_ctx* ctx", "uint64_t* members", "uint64_t* proven", "uint64_t* segments", "uint32_t* batches", "uint64_t* pending_bytes",
        "uint32_t* rounds", "int* serial"]
    for name in ("zz_decode_members_points_device", "zz_ctx_last_decode_members_points_stats"):
        assert hasattr(zz.lib, name), name
    assert "not part of the library yet" not in text


def test_argument_errors_before_anything_is_launched():
    """None of them launches anything, so a block of zeros stands in for a context here; the rows and the destination stay what
    they were."""
    L = zz.lib
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = src = ctypes.cast(fake, ctypes.c_void_p)
    rows = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    R = ctypes.cast(rows, ctypes.c_void_p)
    room = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    dst = ctypes.cast(room, ctypes.c_void_p)
    n = u64(77)

    def decode(c=ctx, s=src, slen=100, d=dst, cap=64, o=ctypes.byref(n), p=R, entries=4, batch=0):
        n.value = 77
        return L.zz_decode_members_points_device(c, s, slen, d, cap, o, p, entries, batch, None)
    assert decode(c=None) == zz.E_ARG and n.value == ERR
    assert decode(o=None) == zz.E_ARG and b"out_len" in L.zz_last_error()
    assert decode(s=None) == zz.E_ARG and n.value == ERR and b"source" in L.zz_last_error()
    assert decode(d=None) == zz.E_ARG and n.value == ERR and b"destination" in L.zz_last_error()
    assert decode(p=None) == zz.E_ARG and n.value == ERR and b"points" in L.zz_last_error()
    assert decode(p=None, entries=1) == zz.E_ARG
    assert decode(entries=1) == zz.E_ARG and n.value == ERR and b"two rows" in L.zz_last_error()
    for batch in ((64 << 20) + 1, 1 << 40, ERR):
        assert decode(batch=batch) == zz.E_ARG and n.value == ERR and b"batch_bytes" in L.zz_last_error(), batch
    # an empty file is zz_decode_members_device's verdict, with rows or without, before anything is launched
    assert decode(s=None, slen=0) == zz.E_DATA and n.value == ERR and b"empty" in L.zz_last_error()
    assert decode(slen=0, p=None, entries=0, d=None, cap=0) == zz.E_DATA and n.value == ERR
    assert rows.raw == b"\xEE" * 64 and room.raw == b"\xEE" * 64

    m, p, s, pend = u64(7), u64(7), u64(7), u64(7)
    b, r, ser = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_int(7)
    assert L.zz_ctx_last_decode_members_points_stats(None, None, None, None, None, None, None, None) == zz.E_ARG
    assert L.zz_ctx_last_decode_members_points_stats(ctx, ctypes.byref(m), ctypes.byref(p), ctypes.byref(s), ctypes.byref(b), ctypes.byref(pend),
                                                     ctypes.byref(r), ctypes.byref(ser)) == 0
    assert (m.value, p.value, s.value, b.value, pend.value, r.value, ser.value) == (0, 0, 0, 0, 0, 0, 0), "nothing ran"
    assert L.zz_ctx_last_decode_members_points_stats(ctx, None, None, None, None, None, None, None) == 0


class FakeContext:
    """what the wrapper touches in front of the library call, without a device"""
    device = 0
    _h = None
    _ptr = staticmethod(zz.Context._ptr)

    def _stream(self):
        return 0


def test_python_wrappers():
    sig = inspect.signature(zz.Context.decode_members_points)
    assert list(sig.parameters) == ["self", "src", "points", "cap", "src_len", "dst", "batch_bytes", "stream"]
    assert [sig.parameters[k].default for k in ("points", "cap", "src_len", "dst", "batch_bytes", "stream")] == [None, None, None, None, 0, None]
    assert list(inspect.signature(zz.Context.last_decode_members_points_stats).parameters) == ["self"]
    for fn in (zz.Context.decode_members_points, zz.Context.last_decode_members_points_stats):
        assert fn.__doc__ and len(fn.__doc__) > 100


def test_python_wrapper_type_errors():
    import torch
    src = torch.zeros(100, dtype=torch.uint8)
    dst = torch.zeros(64, dtype=torch.uint8)
    call = zz.Context.decode_members_points
    for bad in (torch.zeros(64, dtype=torch.int8), torch.zeros((8, 16), dtype=torch.uint8).t(), bytearray(64)):
        with pytest.raises(TypeError, match="dst must be a contiguous uint8 tensor"):
            call(FakeContext(), src, None, dst=bad)
    for bad in (torch.zeros((4, 2), dtype=torch.int32), torch.zeros(8, dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int64),
                [[0.5, 1.0]]):
        with pytest.raises(TypeError, match="points must be"):
            call(FakeContext(), src, bad, dst=dst)
