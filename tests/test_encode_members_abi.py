"""The members encode entry points of the C ABI (include/zzflate_amd.h): declared, exported, refused without a device where they
can be, and mirrored on Context."""
import ctypes
import inspect
import os
import re

import zzflate_amd as zz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(text, result, name):
    m = re.search(r"%s\s+%s\s*\(([^;]*)\);" % (result, name), text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    assert declared(text, "int", "zz_encode_members_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t n", "void* d_dst", "uint64_t cap", "uint64_t* out_len", "int level",
        "uint32_t block_size", "uint32_t packet_size", "int flags", "uint64_t* d_member_offsets", "uint64_t max_offsets",
        "void* hip_stream"]
    assert declared(text, "uint64_t", "zz_encode_members_bound") == ["uint64_t n", "uint32_t block_size", "uint32_t packet_size", "int flags"]
    assert declared(text, "int", "zz_members_header") == ["uint32_t member_bytes", "uint8_t out[18]"]
    assert declared(text, "int", "zz_ctx_last_encode_members_stats") == ["const zz_ctx* ctx", "uint64_t* members", "uint64_t* stored_members"]
    assert re.search(r"enum\s*\{\s*ZZ_MEMBERS_NO_EOF\s*=\s*1\s*\}", text)
    for name in ("zz_encode_members_device", "zz_encode_members_bound", "zz_members_header", "zz_ctx_last_encode_members_stats"):
        assert hasattr(zz.lib, name), name


def test_argument_errors_are_refused_without_a_device():
    L = zz.lib
    out = ctypes.c_uint64(7)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # a null context, whatever else is passed; *out_len = ~0 where there is one
    assert L.zz_encode_members_device(None, p, 64, p, 64, ctypes.byref(out), 1, 0, 0, 0, None, 0, None) == zz.E_ARG
    assert out.value == (1 << 64) - 1
    assert b"null" in L.zz_last_error()
    assert L.zz_encode_members_device(None, None, 0, None, 0, None, 1, 0, 0, 0, None, 0, None) == zz.E_ARG
    assert L.zz_ctx_last_encode_members_stats(None, None, None) == zz.E_ARG
    assert bytes(buf) == bytes(64)


def test_context_has_encode_members():
    sig = inspect.signature(zz.Context.encode_members)
    assert list(sig.parameters) == ["self", "src", "n", "dst", "cap", "level", "block_size", "packet_size", "eof", "offsets", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["level"], d["block_size"], d["packet_size"], d["eof"], d["offsets"], d["stream"]) == (1, 65280, 32768, True, None, None)
    assert list(inspect.signature(zz.Context.last_encode_members_stats).parameters) == ["self"]
    assert zz.MEMBERS_BLOCK == 65280 and zz.DEFAULT_PACKET == 32768
    assert list(inspect.signature(zz.members_bound).parameters) == ["n", "block_size", "packet_size", "eof"]
    assert list(inspect.signature(zz.members_header).parameters) == ["member_bytes"]
    assert list(inspect.signature(zz.gzi_bytes).parameters) == ["offsets", "n", "block_size"]
    # the neighbours' signatures are what they were
    assert list(inspect.signature(zz.Context.encode_batch).parameters) == ["self", "srcs", "dsts", "format", "level", "packet_size", "caps", "stream"]
    assert list(inspect.signature(zz.Context.decode_members).parameters) == ["self", "src", "src_len", "dst", "cap", "stream"]
    assert list(inspect.signature(zz.Context.encode).parameters) == ["self", "src", "n", "dst", "cap", "format", "level", "packet_size", "stream"]
