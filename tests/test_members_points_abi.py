"""The member point index in the C ABI (include/zzflate_amd.h): zz_members_points_device, its stats call and the host helper
zz_members_points_to_index declared and exported, the argument errors that need no device in the shape of the neighbouring calls
(zz_points_index_device, zz_members_find_device), the size protocol of the host helper,
the helper against the case list, and the Python mirror. What needs a device is in tests/test_gpu_members_points.py."""
import ctypes
import inspect
import os
import re

import pytest

import zzflate_amd as zz
import members_find_cases as fc
import members_points_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64
ERR = (1 << 64) - 1


def header():
    return open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()


def args_of(text, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_declared_and_exported():
    text = header()
    assert args_of(text, "zz_members_points_device") == [
        "zz_ctx* ctx", "const void* d_src", "uint64_t src_len", "uint64_t chunk_bytes", "uint64_t spacing", "uint64_t* points",
        "uint64_t max_entries", "uint64_t* entries", "uint64_t* out_len", "void* hip_stream"]
    assert args_of(text, "zz_ctx_last_members_points_stats") == [
        "const zz_ctx* ctx", "uint64_t* members", "uint64_t* header_candidates", "uint64_t* block_candidates", "uint64_t* dropped", "uint32_t* rounds"]
    assert args_of(text, "zz_members_points_to_index") == [
        "const uint64_t* points", "uint64_t entries", "uint64_t* index", "uint64_t max_entries", "uint64_t* index_entries"]
    for name in ("zz_members_points_device", "zz_ctx_last_members_points_stats", "zz_members_points_to_index"):
        assert hasattr(zz.lib, name), name
    assert re.search(r"#define ZZ_MP_START \(1ull << 63\)", text) and re.search(r"#define ZZ_MP_END \(1ull << 62\)", text)
    assert (zz.MP_START, zz.MP_END) == (1 << 63, 1 << 62) == (C.START, C.END)


def test_argument_errors_before_anything_is_launched():
    """None of them launches anything, so a block of zeros stands in for a context here; the rows are 0xEE and stay so."""
    L = zz.lib
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = src = ctypes.cast(fake, ctypes.c_void_p)
    rows = ctypes.create_string_buffer(b"\xEE" * 64, 64)
    R = ctypes.cast(rows, ctypes.c_void_p)
    n, total = u64(77), u64(77)

    def index(c=ctx, s=src, slen=100, chunk=16384, spacing=1, p=R, room=4, e=ctypes.byref(n), o=ctypes.byref(total)):
        return L.zz_members_points_device(c, s, slen, chunk, spacing, p, room, e, o, None)
    assert index(c=None) == zz.E_ARG and (n.value, total.value) == (0, 0)
    assert index(e=None) == zz.E_ARG and index(o=None) == zz.E_ARG
    assert index(s=None) == zz.E_ARG and b"source" in L.zz_last_error()
    assert index(p=None) == zz.E_ARG and b"index" in L.zz_last_error()
    for chunk in (0, 1, 15):
        assert index(chunk=chunk) == zz.E_ARG and b"chunk_bytes must be at least 16" in L.zz_last_error()
    assert index(spacing=0) == zz.E_ARG and b"spacing must be at least 1" in L.zz_last_error()
    assert index(slen=1 << 61) == zz.E_ARG
    n.value = total.value = 77
    assert index(s=None, slen=0) == zz.E_DATA and b"empty" in L.zz_last_error() and (n.value, total.value) == (0, 0)
    assert index(slen=0, p=None, room=0, chunk=16) == zz.E_DATA
    assert rows.raw == b"\xEE" * 64

    m, h, b, d, r = u64(7), u64(7), u64(7), u64(7), ctypes.c_uint32(7)
    assert L.zz_ctx_last_members_points_stats(None, None, None, None, None, None) == zz.E_ARG
    assert L.zz_ctx_last_members_points_stats(ctx, ctypes.byref(m), ctypes.byref(h), ctypes.byref(b), ctypes.byref(d), ctypes.byref(r)) == 0
    assert (m.value, h.value, b.value, d.value, r.value) == (0, 0, 0, 0, 0), "nothing ran"
    assert L.zz_ctx_last_members_points_stats(ctx, None, None, None, None, None) == 0


def to_index(rows, room=None):
    room = len(rows) + 1 if room is None else room
    buf = (u64 * (2 * max(room, 1)))(*([0xEEEE] * (2 * max(room, 1))))
    n = u64(77)
    rc = zz.lib.zz_members_points_to_index(C.flat(rows), len(rows), buf, room, ctypes.byref(n))
    return rc, n.value, [[buf[2 * i], buf[2 * i + 1]] for i in range(room)]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return C.build_harness(tmp_path_factory.mktemp("members_points_abi"))


def test_the_host_helper_against_the_list(H):
    for name, f in list(C.valid_cases().items()) + list(C.planted_cases().items()):
        rows = C.h_index(H, f, 4096).rows
        want = fc.true_chain(f)[0]
        rc, n, got = to_index(rows)
        assert (rc, n, got[:n]) == (0, len(want), want), name
        for room in (0, len(want) - 1):                           # the size protocol: the count is set, nothing is written
            rc, n, got = to_index(rows, room)
            assert (rc, n) == (zz.E_NOSPACE, len(want)) and all(v == [0xEEEE, 0xEEEE] for v in got), (name, room)
    rows = C.h_index(H, C.valid_cases()["two large members"], 4096).rows
    L = zz.lib
    n = u64(7)
    assert L.zz_members_points_to_index(None, 2, None, 0, ctypes.byref(n)) == zz.E_ARG and n.value == 0
    assert L.zz_members_points_to_index(C.flat(rows), len(rows), None, 0, None) == zz.E_ARG
    assert L.zz_members_points_to_index(C.flat(rows), len(rows), None, 4, ctypes.byref(n)) == zz.E_ARG
    for kind in ("start_flag_dropped", "end_flag_dropped", "both_flags", "inner_row_flagged", "last_end_row_removed"):
        assert to_index(C.lie(rows, kind, rows))[0] == zz.E_DATA, kind
    assert to_index(rows[:0] + [[5, 0]])[0] == zz.E_DATA


def test_python_wrappers():
    sig = inspect.signature(zz.Context.members_points)
    assert list(sig.parameters) == ["self", "src", "chunk_bytes", "spacing", "src_len", "stream"]
    assert [sig.parameters[k].default for k in ("chunk_bytes", "spacing", "src_len", "stream")] == [zz.POINTS_CHUNK, 1, None, None]
    assert list(inspect.signature(zz.Context.last_members_points_stats).parameters) == ["self"]
    assert list(inspect.signature(zz.members_index_from_points).parameters) == ["points"]
    for fn in (zz.Context.members_points, zz.members_index_from_points):
        assert fn.__doc__ and len(fn.__doc__) > 100
