"""The members decode entry points of the C ABI (include/zzflate_amd.h): declared, exported, refused without a device where they
can be, and mirrored on Context."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    m = re.search(r"int\s+zz_decode_members_device\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "void* d_dst", "uint64_t cap", "uint64_t* out_len",
                    "void* hip_stream"], args
    m = re.search(r"int\s+zz_ctx_last_decode_members_stats\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const zz_ctx* ctx", "uint64_t* members", "uint64_t* candidates", "int* path"], args
    assert hasattr(zz.lib, "zz_decode_members_device") and hasattr(zz.lib, "zz_ctx_last_decode_members_stats")


def test_argument_errors_are_refused_without_a_device():
    L = zz.lib
    out = ctypes.c_uint64(7)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # a null context, whatever else is passed; *out_len = ~0 where there is one
    assert L.zz_decode_members_device(None, p, 64, p, 64, ctypes.byref(out), None) == zz.E_ARG
    assert out.value == (1 << 64) - 1
    assert b"null" in L.zz_last_error()
    assert L.zz_decode_members_device(None, None, 0, None, 0, None, None) == zz.E_ARG
    assert L.zz_decode_members_device(None, None, 64, p, 64, ctypes.byref(out), None) == zz.E_ARG
    assert L.zz_ctx_last_decode_members_stats(None, None, None, None) == zz.E_ARG


def test_context_has_decode_members():
    sig = inspect.signature(zz.Context.decode_members)
    assert list(sig.parameters) == ["self", "src", "src_len", "dst", "cap", "stream"]
    assert sig.parameters["stream"].default is None
    assert list(inspect.signature(zz.Context.last_decode_members_stats).parameters) == ["self"]
    assert (zz.MEMBERS_BLOCKED, zz.MEMBERS_WALKED, zz.MEMBERS_SERIAL) == (1, 2, 3)
    # the neighbours' signatures are what they were
    assert list(inspect.signature(zz.Context.decode_batch).parameters) == ["self", "srcs", "dsts", "format", "caps", "stream"]
