"""The member finder in the C ABI (include/zzflate_amd.h): zz_members_find_device, zz_decode_members_found_device and
zz_ctx_last_members_find_stats declared and exported, the argument errors that need no device in the order their siblings
(zz_members_index_device, zz_decode_members_device) give them, what is refused before anything is launched, and the Python mirror.
What needs a device -- the size protocol on a real file, the verdicts -- is in tests/test_gpu_members_find.py."""
import ctypes
import inspect
import os
import re

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
    assert args_of(text, "zz_members_find_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "uint64_t limit_bytes", "uint64_t* d_index", "uint64_t max_entries",
        "uint64_t* entries", "void* hip_stream"]
    assert args_of(text, "zz_decode_members_found_device") == args_of(text, "zz_decode_members_device")
    assert args_of(text, "zz_ctx_last_members_find_stats") == ["const zz_ctx* ctx", "uint64_t* members", "uint64_t* candidates", "uint64_t* dropped",
                                                              "uint32_t* rounds"]
    for name in ("zz_members_find_device", "zz_decode_members_found_device", "zz_ctx_last_members_find_stats"):
        assert hasattr(zz.lib, name), name
    m = re.search(r"#define ZZ_MEMBERS_FIND_LIMIT_DEFAULT \(1ull << 20\)\s*/\*(.*?)\*/", text)
    assert m and "derived, not tuned" in m.group(1)
    assert "zz_members_find_device below" in text, "zz_members_index_device's comment points to the new call"


def test_argument_errors_before_anything_is_launched():
    """None of them launches anything, so a block of zeros stands in for a context here; the index array is 0xEE and stays so."""
    L = zz.lib
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = src = ctypes.cast(fake, ctypes.c_void_p)
    idx = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    I = ctypes.cast(idx, ctypes.c_void_p)
    n = u64(77)

    def find(c=ctx, s=src, slen=100, limit=0, i=I, room=4, e=ctypes.byref(n)):
        return L.zz_members_find_device(c, s, slen, limit, i, room, e, None)
    assert find(c=None) == zz.E_ARG and b"null ctx" in L.zz_last_error() and n.value == 0
    n.value = 77
    assert find(e=None) == zz.E_ARG and b"entries" in L.zz_last_error()
    assert find(s=None) == zz.E_ARG and b"source" in L.zz_last_error() and n.value == 0
    assert find(i=None) == zz.E_ARG and b"index" in L.zz_last_error()
    for limit in (0, 1, 1 << 40):
        assert find(s=None, slen=0, limit=limit) == zz.E_DATA and b"empty" in L.zz_last_error(), "an empty file, a null source allowed"
        assert find(slen=0, i=None, room=0, limit=limit) == zz.E_DATA
    assert idx.raw == b"\xEE" * 64

    out = u64(77)
    dst = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    D = ctypes.cast(dst, ctypes.c_void_p)

    def dec(c=ctx, s=src, slen=100, d=D, cap=64, o=ctypes.byref(out)):
        return L.zz_decode_members_found_device(c, s, slen, d, cap, o, None)
    assert dec(c=None) == zz.E_ARG and out.value == (1 << 64) - 1
    assert dec(o=None) == zz.E_ARG and b"out_len" in L.zz_last_error()
    assert dec(s=None) == zz.E_ARG and b"source" in L.zz_last_error()
    assert dec(d=None) == zz.E_ARG and b"destination" in L.zz_last_error()
    out.value = 77
    assert dec(s=None, slen=0, d=None, cap=0) == zz.E_DATA and out.value == (1 << 64) - 1
    assert dst.raw == b"\xEE" * 64

    m, c, d, r = u64(7), u64(7), u64(7), ctypes.c_uint32(7)
    assert L.zz_ctx_last_members_find_stats(None, None, None, None, None) == zz.E_ARG
    assert L.zz_ctx_last_members_find_stats(ctx, ctypes.byref(m), ctypes.byref(c), ctypes.byref(d), ctypes.byref(r)) == 0
    assert (m.value, c.value, d.value, r.value) == (0, 0, 0, 0), "nothing ran"
    assert L.zz_ctx_last_members_find_stats(ctx, None, None, None, None) == 0


def test_python_wrappers():
    sig = inspect.signature(zz.Context.members_find)
    assert list(sig.parameters) == ["self", "src", "limit_bytes", "src_len", "stream"]
    assert [sig.parameters[k].default for k in ("limit_bytes", "src_len", "stream")] == [0, None, None]
    sig = inspect.signature(zz.Context.decode_members_found)
    assert list(sig.parameters) == ["self", "src", "cap", "src_len", "dst", "stream"]
    assert [sig.parameters[k].default for k in ("cap", "src_len", "dst", "stream")] == [None, None, None, None]
    assert list(inspect.signature(zz.Context.last_members_find_stats).parameters) == ["self"]
