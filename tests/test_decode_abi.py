"""The decode entry points of the C ABI (include/zzflate_amd.h): declared, exported, and answered without a device where
they can be."""
import ctypes
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    for name in ("zz_decode_device", "zz_packet_index_device", "zz_ctx_last_decode_path", "zz_ctx_last_decode_stats",
                 "zz_ctx_last_decode_index_device"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(zz.lib, name), name


def test_error_and_path_codes():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    assert re.search(r"ZZ_E_DATA\s*=\s*-6\b", text)
    assert re.search(r"ZZ_DECODE_INDEXED\s*=\s*1\s*,\s*ZZ_DECODE_DISCOVERED\s*=\s*2\s*,\s*ZZ_DECODE_SERIAL\s*=\s*3", text)
    assert (zz.E_DATA, zz.E_NOSPACE, zz.E_UNSUPPORTED) == (-6, -2, -5)
    assert (zz.DECODE_INDEXED, zz.DECODE_DISCOVERED, zz.DECODE_SERIAL) == (1, 2, 3)


def test_null_arguments_are_refused_without_a_device():
    L = zz.lib
    out = ctypes.c_uint64(0)
    assert L.zz_decode_device(None, None, 0, None, 0, ctypes.byref(out), 0, 0, None, 0, None) == -4
    assert L.zz_packet_index_device(None, None, 0, None, None) == -4
    assert L.zz_ctx_last_decode_path(None) == 0
    assert L.zz_ctx_last_decode_stats(None, None, None) == -4
    assert L.zz_ctx_last_decode_index_device(None, None, 0, None, None) == -4


def test_build_flags_stay_empty():
    assert zz.lib.zz_build_flags() == b""
