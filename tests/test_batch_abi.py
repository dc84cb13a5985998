"""The batch entry point of the C ABI (include/zzflate_amd.h): declared, exported, refused without a device where it can be,
and mirrored on Context."""
import ctypes
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    m = re.search(r"int\s+zz_encode_batch_device\s*\(([^;]*)\);", text)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[0].startswith("zz_ctx*") and args[-1].startswith("void* hip_stream"), args
    assert hasattr(zz.lib, "zz_encode_batch_device")


def test_null_arguments_are_refused_without_a_device():
    L = zz.lib
    assert L.zz_encode_batch_device(None, 1, None, None, None, None, None, 0, 1, 32768, None) == -4
    assert L.zz_encode_batch_device(None, 0, None, None, None, None, None, 0, 1, 32768, None) == -4
    # arrays that are not null do not make a null context acceptable, nor do null arrays become acceptable with nitems > 0
    arr = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(arr, ctypes.c_void_p)
    assert L.zz_encode_batch_device(None, 4, p, p, p, p, p, 0, 1, 32768, None) == -4
    assert L.zz_encode_batch_device(None, 4, p, None, p, p, p, 0, 1, 32768, None) == -4


def test_context_has_encode_batch():
    import inspect
    sig = inspect.signature(zz.Context.encode_batch)
    assert list(sig.parameters)[:3] == ["self", "srcs", "dsts"]
    for name in ("format", "level", "packet_size", "caps", "stream"):
        assert name in sig.parameters, name
    assert sig.parameters["packet_size"].default == zz.DEFAULT_PACKET and sig.parameters["caps"].default is None
