"""The multi-range decode's entry points in the C ABI (include/zzflate_amd.h): declared with the documented signatures, exported,
every before-launch argument error refused without a device, and mirrored on Context."""
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
    assert declared("zz_decode_ranges_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "uint32_t packet_size", "const uint64_t* d_index",
        "uint64_t entries", "uint64_t nranges", "const uint64_t* d_firsts", "const uint64_t* d_nbytes", "void* const* d_dsts",
        "const uint64_t* d_caps", "uint64_t* d_out_lens", "int32_t* d_status", "void* hip_stream"]
    assert declared("zz_ctx_last_decode_ranges_stats") == [
        "const zz_ctx* ctx", "uint64_t* packets", "uint32_t* attempts", "uint64_t* retried_ranges", "uint32_t* waves"]
    assert hasattr(zz.lib, "zz_decode_ranges_device") and hasattr(zz.lib, "zz_ctx_last_decode_ranges_stats")
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    doc = text[text.index("Many reads of one stored stream in one call"): text.index("int zz_decode_ranges_device")]
    assert "NOT CHECKED" in doc and "checksum" in doc          # the header says what the call does not verify
    assert "Workspace" in doc                                   # and bounds its workspace


def call(ctx, src, idx, firsts, nbytes, dsts, caps, lens, fmt=0, P=1000, entries=5, nranges=3, status=None):
    return zz.lib.zz_decode_ranges_device(ctx, src, 100, fmt, P, idx, entries, nranges, firsts, nbytes, dsts, caps, lens, status, None)


def test_argument_errors_are_refused_without_a_device():
    """none of these reaches the context: a word of host memory stands in for it"""
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    E = zz.E_ARG
    assert call(None, p, p, p, p, p, p, p) == E and b"null" in zz.lib.zz_last_error()
    assert call(p, None, p, p, p, p, p, p) == E and call(p, p, None, p, p, p, p, p) == E
    assert call(p, p, p, None, p, p, p, p) == E and call(p, p, p, p, None, p, p, p) == E
    assert call(p, p, p, p, p, None, p, p) == E and call(p, p, p, p, p, p, None, p) == E
    assert call(p, p, p, p, p, p, p, None) == E and b"null" in zz.lib.zz_last_error()
    assert call(p, p, p, p, p, p, p, p, P=0) == E and call(p, p, p, p, p, p, p, p, P=32769) == E
    assert b"packet size must be 1..32768" in zz.lib.zz_last_error()
    assert call(p, p, p, p, p, p, p, p, fmt=-1) == E and call(p, p, p, p, p, p, p, p, fmt=3) == E
    assert b"format must be" in zz.lib.zz_last_error()
    assert call(p, p, p, p, p, p, p, p, entries=0) == E and call(p, p, p, p, p, p, p, p, entries=1) == E
    assert b"at least two entries" in zz.lib.zz_last_error()
    assert call(p, p, p, p, p, p, p, p, nranges=1 << 31) == E and call(p, p, p, p, p, p, p, p, nranges=(1 << 64) - 1) == E
    assert list(word) == [0] * 8


def test_no_reads_is_ok_at_once():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert call(p, p, p, p, p, p, p, p, nranges=0) == 0
    assert call(p, p, p, p, p, p, p, p, nranges=0, status=p) == 0
    assert call(p, p, p, p, p, p, p, p, nranges=0, P=0) == zz.E_ARG            # the arguments are checked first
    assert list(word) == [0] * 8


def test_stats_need_a_context():
    assert zz.lib.zz_ctx_last_decode_ranges_stats(None, None, None, None, None) == zz.E_ARG


def test_context_has_decode_ranges():
    sig = inspect.signature(zz.Context.decode_ranges)
    assert list(sig.parameters) == ["self", "src", "src_len", "firsts", "nbytes", "dsts", "caps", "format", "packet_size", "index", "stream"]
    assert sig.parameters["caps"].default is None
    assert sig.parameters["format"].default == zz.Format.Zlib and sig.parameters["packet_size"].default == zz.DEFAULT_PACKET
    assert sig.parameters["index"].default is None and sig.parameters["stream"].default is None
    assert list(inspect.signature(zz.Context.last_decode_ranges_stats).parameters) == ["self"]
    # the single read's and the whole-stream decode's signatures are what they were
    rng = inspect.signature(zz.Context.decode_range)
    assert list(rng.parameters) == ["self", "src", "src_len", "dst", "cap", "first", "nbytes", "format", "packet_size", "index", "stream"]
    dec = inspect.signature(zz.Context.decode)
    assert list(dec.parameters) == ["self", "src", "src_len", "dst", "cap", "format", "packet_size", "index", "stream"]
