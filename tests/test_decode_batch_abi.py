"""The batch decode entry point of the C ABI (include/zzflate_amd.h): declared, exported, refused without a device where it
can be, and mirrored on Context."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    m = re.search(r"int\s+zz_decode_batch_device\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0].startswith("zz_ctx*") and args[-1].startswith("void* hip_stream"), args
    assert args[7].startswith("int32_t* d_status") and args[8] == "int format", args
    assert hasattr(zz.lib, "zz_decode_batch_device")


def test_null_arguments_are_refused_without_a_device():
    L = zz.lib
    assert L.zz_decode_batch_device(None, 1, None, None, None, None, None, None, 0, None) == -4
    assert L.zz_decode_batch_device(None, 0, None, None, None, None, None, None, 0, None) == -4
    arr = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    # arrays that are not null do not make a null context acceptable, nor do null arrays become acceptable with nitems > 0
    assert L.zz_decode_batch_device(None, 4, p, p, p, p, p, p, 0, None) == -4
    assert L.zz_decode_batch_device(None, 4, p, None, p, p, p, None, 0, None) == -4
    assert L.zz_decode_batch_device(None, 4, p, p, p, p, p, p, 7, None) == -4
    assert b"null" in L.zz_last_error()


def test_context_has_decode_batch():
    sig = inspect.signature(zz.Context.decode_batch)
    assert list(sig.parameters) == ["self", "srcs", "dsts", "format", "caps", "stream"]
    assert sig.parameters["format"].default == zz.Format.Zlib
    assert sig.parameters["caps"].default is None and sig.parameters["stream"].default is None
    # the batch encode's own signature is what it was
    enc = inspect.signature(zz.Context.encode_batch)
    assert list(enc.parameters) == ["self", "srcs", "dsts", "format", "level", "packet_size", "caps", "stream"]


def test_build_flags_are_empty():
    assert zz.lib.zz_build_flags() == b""
