"""The checked range reads' entry points and the sidecar's producer in the C ABI (include/zzflate_amd.h): declared with the
documented signatures, exported, every before-launch argument error refused without a device, and mirrored on Context."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64
HEADER = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def declared(name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, HEADER)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    assert declared("zz_packet_checksums_device") == [
        "zz_ctx* ctx", "const void* d_data", "uint64_t n", "uint32_t packet_size", "int format", "uint32_t* d_cks",
        "uint64_t max_entries", "uint64_t* entries", "void* hip_stream"]
    assert declared("zz_decode_range_checked_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "uint32_t packet_size", "const uint64_t* d_index",
        "uint64_t entries", "const uint32_t* d_cks", "uint64_t total_len", "uint64_t first", "uint64_t nbytes", "void* d_dst",
        "uint64_t cap", "uint64_t* out_len", "void* hip_stream"]
    assert declared("zz_decode_ranges_checked_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "int format", "uint32_t packet_size", "const uint64_t* d_index",
        "uint64_t entries", "const uint32_t* d_cks", "uint64_t total_len", "uint64_t nranges", "const uint64_t* d_firsts",
        "const uint64_t* d_nbytes", "void* const* d_dsts", "const uint64_t* d_caps", "uint64_t* d_out_lens", "int32_t* d_status",
        "void* hip_stream"]
    for name in ("zz_packet_checksums_device", "zz_decode_range_checked_device", "zz_decode_ranges_checked_device"):
        assert hasattr(zz.lib, name), name
    # the unchecked calls still say what they do not verify, and now where to go for it
    single = HEADER[HEADER.index("Random access into a stored stream"): HEADER.index("int zz_decode_range_device")]
    multi = HEADER[HEADER.index("Many reads of one stored stream in one call"): HEADER.index("int zz_decode_ranges_device")]
    assert "NOT CHECKED" in single and "zz_decode_range_checked_device" in single
    assert "NOT CHECKED" in multi and "zz_decode_ranges_checked_device" in multi
    doc = HEADER[HEADER.index("checked range reads: a per-packet checksum sidecar"): HEADER.index("int zz_decode_ranges_checked_device")]
    assert "ZZ_DEFLATE HAS NO TRAILER" in doc and "caller" in doc          # what a raw stream cannot promise, said plainly


def producer(ctx, data, n, P, fmt, cks, max_entries, entries):
    return zz.lib.zz_packet_checksums_device(ctx, data, n, P, fmt, cks, max_entries, entries, None)


def test_producer_argument_errors_without_a_device():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    n = u64(77)
    e = ctypes.byref(n)
    E = zz.E_ARG
    assert producer(None, p, 10, 1000, 0, p, 1, e) == E and b"null" in zz.lib.zz_last_error()
    assert producer(p, p, 10, 1000, 0, p, 1, None) == E and producer(p, p, 10, 1000, 0, None, 1, e) == E
    assert producer(p, None, 10, 1000, 0, p, 1, e) == E
    assert producer(p, p, 10, 0, 0, p, 1, e) == E and producer(p, p, 10, 32769, 0, p, 1, e) == E
    assert b"packet size must be 1..32768" in zz.lib.zz_last_error()
    assert producer(p, p, 10, 1000, -1, p, 1, e) == E and producer(p, p, 10, 1000, 3, p, 1, e) == E
    assert producer(p, p, 1 << 31, 1, 0, p, 1 << 40, e) == E and b"2^31 - 1 packets" in zz.lib.zz_last_error()
    assert n.value == 77
    # too small a buffer: the count comes back, nothing is written, the context is not looked at
    assert producer(p, p, 3017, 1000, 0, p, 3, e) == zz.E_NOSPACE and n.value == 4
    assert producer(p, p, 0, 1000, 1, p, 0, e) == zz.E_NOSPACE and n.value == 1
    assert producer(p, p, (1 << 31) - 1, 1, 2, p, 5, e) == zz.E_NOSPACE and n.value == (1 << 31) - 1
    assert list(word) == [0] * 8


def single(ctx, src, idx, cks, out, fmt=0, P=1000, entries=5, total_len=3500, first=0, nbytes=10, dst=None, cap=0):
    return zz.lib.zz_decode_range_checked_device(ctx, src, 100, fmt, P, idx, entries, cks, total_len, first, nbytes, dst, cap, out, None)


def test_single_read_argument_errors_without_a_device():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    n = u64(77)
    o = ctypes.byref(n)
    E = zz.E_ARG
    assert single(None, p, p, p, o) == E and single(p, None, p, p, o) == E and single(p, p, None, p, o) == E
    assert single(p, p, p, p, None) == E
    assert single(p, p, p, None, o) == E and b"null" in zz.lib.zz_last_error()             # the sidecar
    assert single(p, p, p, p, o, P=0) == E and single(p, p, p, p, o, P=32769) == E
    assert single(p, p, p, p, o, fmt=3) == E and single(p, p, p, p, o, entries=1) == E
    assert single(p, p, p, p, o, first=4000) == E and single(p, p, p, p, o, first=5, nbytes=(1 << 64) - 3) == E
    assert single(p, p, p, p, o, cap=5) == E                                                # a null destination with room
    for total_len in (0, 3000, 4001, 1 << 40):                                              # not four packets of 1000
        assert single(p, p, p, p, o, total_len=total_len) == E, total_len
        assert b"total_len" in zz.lib.zz_last_error()
    assert single(p, p, p, p, o, entries=2, total_len=0, nbytes=0) == 0                     # an empty stream has one packet
    assert single(p, p, p, p, o, entries=3, total_len=0, nbytes=0) == E
    assert single(p, p, p, p, o, P=1, entries=(1 << 31) + 1, total_len=1 << 31) == E and b"2^31 - 1 packets" in zz.lib.zz_last_error()
    assert single(p, p, p, p, o, total_len=3001, nbytes=0) == 0 and n.value == 0            # arguments pass, nothing to do
    assert list(word) == [0] * 8


def multi(ctx, src, idx, cks, firsts, nbytes, dsts, caps, lens, fmt=0, P=1000, entries=5, total_len=3500, nranges=3, status=None):
    return zz.lib.zz_decode_ranges_checked_device(ctx, src, 100, fmt, P, idx, entries, cks, total_len, nranges, firsts, nbytes, dsts,
                                                  caps, lens, status, None)


def test_multi_read_argument_errors_without_a_device():
    word = (u64 * 8)()
    p = ctypes.cast(word, ctypes.c_void_p)
    E = zz.E_ARG
    assert multi(None, p, p, p, p, p, p, p, p) == E and multi(p, None, p, p, p, p, p, p, p) == E
    assert multi(p, p, None, p, p, p, p, p, p) == E and multi(p, p, p, p, None, p, p, p, p) == E
    assert multi(p, p, p, p, p, None, p, p, p) == E and multi(p, p, p, p, p, p, None, p, p) == E
    assert multi(p, p, p, p, p, p, p, None, p) == E and multi(p, p, p, p, p, p, p, p, None) == E
    assert multi(p, p, p, None, p, p, p, p, p) == E and b"null" in zz.lib.zz_last_error()   # the sidecar
    assert multi(p, p, p, p, p, p, p, p, p, P=0) == E and multi(p, p, p, p, p, p, p, p, p, fmt=-1) == E
    assert multi(p, p, p, p, p, p, p, p, p, entries=1) == E and multi(p, p, p, p, p, p, p, p, p, nranges=1 << 31) == E
    for total_len in (0, 3000, 4001):
        assert multi(p, p, p, p, p, p, p, p, p, total_len=total_len) == E and b"total_len" in zz.lib.zz_last_error()
    assert multi(p, p, p, p, p, p, p, p, p, nranges=0) == 0
    assert multi(p, p, p, p, p, p, p, p, p, nranges=0, total_len=3000) == E                 # the arguments are checked first
    assert list(word) == [0] * 8


def test_context_has_the_checked_calls():
    """the unchecked methods keep their signatures (tests/test_decode_ranges_abi.py pins them); the checked reads are methods of
    their own with the sidecar and the decoded length as required arguments"""
    sig = inspect.signature(zz.Context.decode_range_checked)
    assert list(sig.parameters) == ["self", "src", "src_len", "dst", "cap", "first", "nbytes", "checksums", "total_len", "format",
                                    "packet_size", "index", "stream"]
    sig = inspect.signature(zz.Context.decode_ranges_checked)
    assert list(sig.parameters) == ["self", "src", "src_len", "firsts", "nbytes", "dsts", "checksums", "total_len", "caps", "format",
                                    "packet_size", "index", "stream"]
    sig = inspect.signature(zz.Context.packet_checksums)
    assert list(sig.parameters) == ["self", "data", "n", "format", "packet_size", "stream"]
    assert list(inspect.signature(zz.packet_checksums_host).parameters) == ["data", "format", "packet_size"]
