"""The range decode's entry points in the C ABI (include/zzflate_amd.h): declared with the documented signatures, exported,
every argument error refused without a device, and mirrored on Context."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64


def declared(name):
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    assert declared("zz_decode_range_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "uint32_t packet_size", "const uint64_t* d_index",
        "uint64_t entries", "uint64_t first", "uint64_t nbytes", "void* d_dst", "uint64_t cap", "uint64_t* out_len", "void* hip_stream"]
    assert declared("zz_ctx_last_decode_range_stats") == [
        "const zz_ctx* ctx", "uint64_t* first_packet", "uint64_t* packets", "uint32_t* attempts", "uint64_t* pending_bytes"]
    assert hasattr(zz.lib, "zz_decode_range_device") and hasattr(zz.lib, "zz_ctx_last_decode_range_stats")
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    doc = text[text.index("Random access into a stored stream"): text.index("int zz_decode_range_device")]
    assert "NOT CHECKED" in doc and "checksum" in doc          # the header says what the call does not verify


def call(ctx, src, idx, out, fmt=0, P=1000, entries=5, first=0, nbytes=1, dst=None, cap=0):
    return zz.lib.zz_decode_range_device(ctx, src, 100, fmt, P, idx, entries, first, nbytes, dst, cap, out, None)


def test_argument_errors_are_refused_without_a_device():
    """none of these reaches the context: a word of host memory stands in for it"""
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    out = u64(7)
    o = ctypes.byref(out)
    E = zz.E_ARG
    assert call(None, p, p, o) == E and b"null" in zz.lib.zz_last_error()
    assert call(p, None, p, o) == E and call(p, p, None, o) == E and call(p, p, p, None) == E
    assert call(p, p, p, o, P=0) == E and call(p, p, p, o, P=32769) == E
    assert call(p, p, p, o, fmt=-1) == E and call(p, p, p, o, fmt=3) == E
    assert call(p, p, p, o, entries=0) == E and call(p, p, p, o, entries=1) == E
    assert call(p, p, p, o, first=4000) == E and call(p, p, p, o, first=(1 << 64) - 1) == E      # first >= (entries - 1) * P
    assert call(p, p, p, o, entries=2, P=32768, first=32768) == E
    assert call(p, p, p, o, first=3999, nbytes=(1 << 64) - 3999) == E                            # first + nbytes overflows
    assert call(p, p, p, o, first=1, nbytes=(1 << 64) - 1) == E
    assert out.value == 0


def test_an_empty_range_is_ok_at_once():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    out = u64(7)
    assert call(p, p, p, ctypes.byref(out), nbytes=0) == 0 and out.value == 0
    assert call(p, p, p, ctypes.byref(out), first=3999, nbytes=0) == 0 and out.value == 0
    assert call(p, p, p, ctypes.byref(out), first=4000, nbytes=0) == zz.E_ARG                    # the arguments are checked first


def test_stats_need_a_context():
    assert zz.lib.zz_ctx_last_decode_range_stats(None, None, None, None, None) == zz.E_ARG


def test_context_has_decode_range():
    sig = inspect.signature(zz.Context.decode_range)
    assert list(sig.parameters) == ["self", "src", "src_len", "dst", "cap", "first", "nbytes", "format", "packet_size", "index", "stream"]
    assert sig.parameters["format"].default == zz.Format.Zlib and sig.parameters["packet_size"].default == zz.DEFAULT_PACKET
    assert sig.parameters["index"].default is None and sig.parameters["stream"].default is None
    assert list(inspect.signature(zz.Context.last_decode_range_stats).parameters) == ["self"]
    # the whole-stream decode's signature is what it was
    dec = inspect.signature(zz.Context.decode)
    assert list(dec.parameters) == ["self", "src", "src_len", "dst", "cap", "format", "packet_size", "index", "stream"]
