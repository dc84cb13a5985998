"""The indexed reads of blocked gzip files in the C ABI (include/zzflate_amd.h): the three entry points are declared with the
documented signatures and exported, every before-launch argument error is refused without a device, the Context methods and
the module function have the stated parameters, and the neighbours' signatures are what they were."""
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
    assert declared("zz_members_index_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "uint64_t* d_index", "uint64_t max_entries", "uint64_t* entries",
        "void* hip_stream"]
    assert declared("zz_decode_members_ranges_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "const uint64_t* d_index", "uint64_t entries", "uint64_t nranges",
        "const uint64_t* d_firsts", "const uint64_t* d_nbytes", "void* const* d_dsts", "const uint64_t* d_caps", "uint64_t* d_out_lens",
        "int32_t* d_status", "void* hip_stream"]
    assert declared("zz_ctx_last_decode_members_ranges_stats") == ["const zz_ctx* ctx", "uint64_t* members_decoded", "uint32_t* waves"]
    for name in ("zz_members_index_device", "zz_decode_members_ranges_device", "zz_ctx_last_decode_members_ranges_stats"):
        assert hasattr(zz.lib, name), name
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    doc = text[text.index("Many reads of one blocked gzip (BGZF) file"): text.index("int zz_decode_members_ranges_device")]
    assert "CHECKED COMPLETELY" in doc and "CRC-32" in doc and "ISIZE" in doc      # the header says what a read verifies
    assert "Workspace" in doc and "28 bytes per member" in doc                     # and states its workspace
    doc = text[text.index("The index of a blocked gzip (BGZF) file"): text.index("int zz_members_index_device")]
    assert "NOTHING IS DECODED" in doc and "zz_decode_members_device" in doc       # a file that is not blocked is sent there


def call(ctx, src, idx, firsts, nbytes, dsts, caps, lens, entries=5, nranges=3, status=None):
    return zz.lib.zz_decode_members_ranges_device(ctx, src, 100, idx, entries, nranges, firsts, nbytes, dsts, caps, lens, status, None)


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
    assert call(p, p, p, p, p, p, p, p, entries=0) == E and call(p, p, p, p, p, p, p, p, entries=1) == E
    assert b"at least two entries" in zz.lib.zz_last_error()
    assert call(p, p, p, p, p, p, p, p, entries=(1 << 31) + 1) == E and call(p, p, p, p, p, p, p, p, entries=(1 << 64) - 1) == E
    assert b"members" in zz.lib.zz_last_error()
    assert call(p, p, p, p, p, p, p, p, nranges=1 << 31) == E and call(p, p, p, p, p, p, p, p, nranges=(1 << 64) - 1) == E
    assert list(word) == [0] * 8


def test_no_reads_is_ok_at_once():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert call(p, p, p, p, p, p, p, p, nranges=0) == 0
    assert call(p, p, p, p, p, p, p, p, nranges=0, status=p) == 0
    assert call(p, p, p, p, p, p, p, p, nranges=0, entries=1 << 31) == 0          # 2^31 - 1 members are the most an index holds
    assert call(p, p, p, p, p, p, p, p, nranges=0, entries=1) == zz.E_ARG           # the arguments are checked first
    assert list(word) == [0] * 8


def test_index_call_refuses_null_arguments_without_a_device():
    n = u64(7)
    assert zz.lib.zz_members_index_device(None, None, 0, None, 0, ctypes.byref(n), None) == zz.E_ARG and n.value == 0
    assert b"null" in zz.lib.zz_last_error()
    assert zz.lib.zz_members_index_device(None, None, 0, None, 0, None, None) == zz.E_ARG


def test_stats_need_a_context():
    assert zz.lib.zz_ctx_last_decode_members_ranges_stats(None, None, None) == zz.E_ARG


def test_python_interface():
    sig = inspect.signature(zz.Context.decode_members_ranges)
    assert list(sig.parameters) == ["self", "src", "src_len", "index", "firsts", "nbytes", "dsts", "caps", "stream"]
    assert sig.parameters["caps"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(zz.Context.members_index)
    assert list(sig.parameters) == ["self", "src", "src_len", "stream"] and sig.parameters["stream"].default is None
    assert list(inspect.signature(zz.Context.last_decode_members_ranges_stats).parameters) == ["self"]
    sig = inspect.signature(zz.members_index_from_offsets)
    assert list(sig.parameters) == ["offsets", "n", "block_size", "eof"]
    assert sig.parameters["block_size"].default == zz.MEMBERS_BLOCK and sig.parameters["eof"].default is True


def test_the_neighbours_are_what_they_were():
    assert declared("zz_decode_members_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "void* d_dst", "uint64_t cap", "uint64_t* out_len", "void* hip_stream"]
    assert declared("zz_ctx_last_decode_members_stats") == ["const zz_ctx* ctx", "uint64_t* members", "uint64_t* candidates", "int* path"]
    assert declared("zz_decode_ranges_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "uint32_t packet_size", "const uint64_t* d_index",
        "uint64_t entries", "uint64_t nranges", "const uint64_t* d_firsts", "const uint64_t* d_nbytes", "void* const* d_dsts",
        "const uint64_t* d_caps", "uint64_t* d_out_lens", "int32_t* d_status", "void* hip_stream"]
    assert declared("zz_packet_index_device") == ["zz_ctx* ctx", "uint64_t* d_index", "uint64_t max_entries", "uint64_t* entries", "void* hip_stream"]
    assert list(inspect.signature(zz.Context.decode_members).parameters) == ["self", "src", "src_len", "dst", "cap", "stream"]
    assert list(inspect.signature(zz.Context.decode_ranges).parameters) == [
        "self", "src", "src_len", "firsts", "nbytes", "dsts", "caps", "format", "packet_size", "index", "stream"]
    assert list(inspect.signature(zz.Context.encode_members).parameters) == [
        "self", "src", "n", "dst", "cap", "level", "block_size", "packet_size", "eof", "offsets", "stream"]
    assert list(inspect.signature(zz.gzi_bytes).parameters) == ["offsets", "n", "block_size"]
