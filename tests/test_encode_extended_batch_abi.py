"""The extended levels' switch of the batch and members encode calls in the C ABI (include/zzflate_amd.h): the new entry point is
declared and exported, the constants agree between the header and Python, and what can be refused without a device is."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def declared(result, name):
    m = re.search(r"%s\s+%s\s*\(([^;]*)\);" % (result, name), HEADER)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def enum_value(name):
    m = re.search(r"enum\s*\{[^}]*\b%s\s*=\s*(\d+)[^}]*\}" % name, HEADER)
    assert m, name
    return int(m.group(1))


def test_the_flags_entry_point_is_declared_and_exported():
    batch = declared("int", "zz_encode_batch_device")
    assert declared("int", "zz_encode_batch_flags_device") == batch[:-1] + ["int flags", "void* hip_stream"]
    assert batch[-1] == "void* hip_stream" and len(batch) == 11
    assert hasattr(zz.lib, "zz_encode_batch_flags_device")
    f = zz.lib.zz_encode_batch_flags_device
    assert f.restype is ctypes.c_int32 or f.restype is ctypes.c_int
    assert len(f.argtypes) == 12 and f.argtypes[10] in (ctypes.c_int32, ctypes.c_int)


def test_constants_agree():
    assert enum_value("ZZ_BATCH_EXTENDED") == zz.BATCH_EXTENDED == 1
    assert enum_value("ZZ_MEMBERS_EXTENDED") == zz.MEMBERS_EXTENDED == 2
    assert enum_value("ZZ_MEMBERS_NO_EOF") == zz.MEMBERS_NO_EOF == 1
    assert zz.MEMBERS_EXTENDED & zz.MEMBERS_NO_EOF == 0


def test_a_null_context_is_refused_without_a_device():
    L = zz.lib
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for flags in (0, zz.BATCH_EXTENDED, 2):
        assert L.zz_encode_batch_flags_device(None, 4, p, p, p, p, p, 0, 6, 32768, flags, None) == zz.E_ARG
        assert b"null" in L.zz_last_error()
    out = ctypes.c_uint64(7)
    assert L.zz_encode_members_device(None, p, 64, p, 64, ctypes.byref(out), 6, 0, 0, zz.MEMBERS_EXTENDED, None, 0, None) == zz.E_ARG
    assert out.value == (1 << 64) - 1
    assert bytes(buf) == bytes(64)


def test_the_bound_does_not_depend_on_the_switch():
    L = zz.lib
    for n in (0, 1, 65280, 65281, 1 << 20, (1 << 30) + 5):
        for B, P in ((0, 0), (65280, 4096), (8192, 4096), (777, 300)):
            for eof in (0, zz.MEMBERS_NO_EOF):
                assert L.zz_encode_members_bound(n, B, P, eof) == L.zz_encode_members_bound(n, B, P, eof | zz.MEMBERS_EXTENDED)
    assert L.zz_encode_members_bound(100, 65280, 1000, zz.MEMBERS_EXTENDED) == (1 << 64) - 1       # sizes the call refuses, still refused


def test_context_has_the_extended_methods():
    b = inspect.signature(zz.Context.encode_batch_extended)
    assert list(b.parameters) == list(inspect.signature(zz.Context.encode_batch).parameters)
    m = inspect.signature(zz.Context.encode_members_extended)
    assert list(m.parameters) == list(inspect.signature(zz.Context.encode_members).parameters)
    assert b.parameters["level"].default == 6 and m.parameters["level"].default == 6          # bgzip's default
