"""zz_points_index_device / Context.points_index / Context.decode_found: the point index of a stream met for the first time, built
on the device. Every stream goes through the bounds-checked CPU harness first (tests/points_find_cases.py,
tests/cxx/points_find_harness.cpp): the result is defined by the stream, the chunk size and the spacing alone, so the device's
rows, its decoded length and its stats -- candidates, dropped candidates and rounds -- equal the harness's exactly. Then
decode_points takes each index: it never trusts one, so the original bytes on the points path prove the rows honest.
Needs a real MI355X: run with `-m gpu`."""
import ctypes
import zlib

import pytest

import points_cases as pc
import points_find_cases as fc
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
u64 = ctypes.c_uint64
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return fc.build_harness(tmp_path_factory.mktemp("points_find"))


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def index(torch, ctx, src, n, fmt, chunk, spacing=1, max_entries=None):
    """the call itself: a fc.Found, the rows between guard values that must stay what they were"""
    cap = zz.points_index_bound(n, chunk) if max_entries is None else max_entries
    buf = (u64 * (2 * cap + 4))(*([GUARD] * (2 * cap + 4)))
    e, m = u64(0), u64(0)
    rc = zz.lib.zz_points_index_device(ctx._h, src.data_ptr(), n, int(fmt), chunk, spacing, ctypes.byref(buf, 16), cap,
                                       ctypes.byref(e), ctypes.byref(m), None)
    assert buf[0] == buf[1] == GUARD and buf[2 * cap + 2] == buf[2 * cap + 3] == GUARD, "rows outside the buffer were written"
    rows = [[buf[2 + 2 * i], buf[3 + 2 * i]] for i in range(e.value)] if rc == 0 else []
    if rc != 0:
        assert all(v == GUARD for v in buf), "a refused call wrote rows"
    return fc.Found(rc, rows, m.value, e.value, list(ctx.last_points_index_stats()) + [0])


def decode_with(torch, ctx, src, n, fmt, rows, data):
    """decode_points with these rows: the original bytes on the points path"""
    dst = torch.full((len(data) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    points = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
    assert ctx.decode_points(src, n, dst, len(data), points, fmt) == len(data)
    host = dst.cpu().numpy().tobytes()
    assert host[: len(data)] == data and host[len(data):] == b"\xEE" * 64
    assert ctx.last_decode_path() == zz.DECODE_POINTS


@pytest.mark.parametrize("name", fc.CLEAN)
def test_clean_streams(torch, ctx, H, name):
    s, fmt, data = pc.case(name)
    src = dev(torch, s)
    for chunk in fc.chunks_of(name):
        want = fc.h_index(H, s, fmt, chunk)
        got = index(torch, ctx, src, len(s), fmt, chunk)
        print(f"{name} chunk {chunk}: {got.candidates} candidates, {got.dropped} dropped, {got.rounds} rounds, {len(got.rows)} rows")
        assert want.rc == 0 and got.key() == want.key(), (name, chunk)
        assert got.out_len == len(data)
        decode_with(torch, ctx, src, len(s), fmt, got.rows, data)
    # the Python face, thinned, and the index and the decode in one call
    points, n = ctx.points_index(src, len(s), fmt, fc.chunks_of(name)[0], 4096)
    assert n == len(data) and points.tolist() == fc.h_index(H, s, fmt, fc.chunks_of(name)[0], spacing=4096).rows
    assert points.dtype == torch.int64 and points.device.type == "cpu"
    decode_with(torch, ctx, src, len(s), fmt, points.tolist(), data)
    dst = torch.full((len(data) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert ctx.decode_found(src, len(s), dst, len(data), fmt, 4096) == len(data)
    assert dst.cpu().numpy().tobytes() == data + b"\xEE" * 64 and ctx.last_decode_path() == zz.DECODE_POINTS


@pytest.mark.parametrize("name", tuple(fc.PLANTED))
def test_planted_headers_are_dropped(torch, ctx, H, name):
    s, fmt, data, planted_bits = fc.planted(name)
    src = dev(torch, s)
    for chunk in fc.PLANTED[name][2]:
        want = fc.h_index(H, s, fmt, chunk)
        got = index(torch, ctx, src, len(s), fmt, chunk)
        print(f"{name} chunk {chunk}: {got.candidates} candidates, {got.dropped} dropped, {got.rounds} rounds")
        assert got.key() == want.key()
        assert got.dropped >= len(planted_bits) and got.rounds >= 2 and not set(planted_bits) & {r[0] for r in got.rows}
        decode_with(torch, ctx, src, len(s), fmt, got.rows, data)


def test_edges_of_the_chunking(torch, ctx, H):
    """a true header in a chunk's last bits, one at a chunk's first bit, a final block alone in the last chunk (the premises are
    asserted in tests/test_points_find_cpu.py): here every chunk size of a stretch, against the harness"""
    s, fmt, data = pc.case("alice_mem1")
    src = dev(torch, s)
    for chunk in list(range(64, 128, 3)) + [271, 1094]:
        got = index(torch, ctx, src, len(s), fmt, chunk)
        assert got.key() == fc.h_index(H, s, fmt, chunk).key(), chunk
    decode_with(torch, ctx, src, len(s), fmt, got.rows, data)
    # a dynamic header cut off by the stream's end in a chunk's first bits: refused, as the harness refuses it
    raw = pc.case("alice_raw")[0]
    front = b"\x00" + fc.struct.pack("<HH", 59, 59 ^ 0xFFFF) + bytes(59)
    for n in range(20, 120, 7):
        t = front + raw[:n]
        got = index(torch, ctx, dev(torch, t), len(t), pc.RAW, 64)
        assert got.key() == fc.h_index(H, t, pc.RAW, 64).key() and got.rc == zz.E_DATA, n


def test_one_row_too_few(torch, ctx, H):
    s, fmt, data = pc.case("alice_mem1")
    src = dev(torch, s)
    want = fc.h_index(H, s, fmt, 1000)
    for cap in (want.entries - 1, 1, 0):
        got = index(torch, ctx, src, len(s), fmt, 1000, max_entries=cap)          # (index() asserts that nothing was written)
        assert (got.rc, got.entries, got.out_len) == (zz.E_NOSPACE, want.entries, len(data)), cap
    assert index(torch, ctx, src, len(s), fmt, 1000, max_entries=want.entries).key() == want.key()
    e, m = u64(0), u64(0)
    assert zz.lib.zz_points_index_device(ctx._h, src.data_ptr(), len(s), int(fmt), 1000, 1, None, 1 << 20, ctypes.byref(e), ctypes.byref(m), None) == zz.E_NOSPACE
    assert (e.value, m.value) == (want.entries, len(data)), "a null rows pointer asks for the count"


@pytest.mark.parametrize("part", range(4))
def test_damaged_streams(torch, ctx, H, part):
    """the 200 flips and the truncations of alice_l6, a quarter each (both kinds of result are in the list: test_points_find_cpu.py)"""
    streams, fmt = fc.damaged("alice_l6")
    for s in streams[part::4]:
        src = dev(torch, s)
        want = fc.h_index(H, s, fmt, 1000)
        got = index(torch, ctx, src, len(s), fmt, 1000)
        assert got.rc == want.rc and got.rc in (0, zz.E_DATA, zz.E_UNSUPPORTED)
        if got.rc != 0:
            continue
        assert got.key() == want.key()
        v = pc.zlib_verdict(s, fmt)                              # decode_points with that index gives zlib's verdict
        cap = max(got.out_len, len(v) if v is not None else 0)
        dst = torch.zeros(cap + 1, dtype=torch.uint8, device="cuda")
        points = torch.tensor(got.rows, dtype=torch.int64).reshape(-1, 2)
        try:
            n = ctx.decode_points(src, len(s), dst, cap, points, fmt)
            assert v is not None and dst[:n].cpu().numpy().tobytes() == v
        except zz.ZzFlateError as err:
            assert v is None and err.code == zz.E_DATA


@pytest.mark.parametrize("name", ("periodic_mem1_raw", "mix_mem1"))
def test_many_chunks_in_one_launch(torch, ctx, H, name):
    """the smallest chunks there are, 16 bytes. Chunks are COMPRESSED bytes: the 3 MiB periodic stream is 4,257 of them (266
    chunks, a third of them with a block start), the 1.4 MB mix at memLevel 1 375,252: 23,453 chunks for 4,096 persistent
    wavefronts in one launch, and 1,913 jobs in the next -- the counters that deal them out"""
    s, fmt, data = pc.case(name)
    src = dev(torch, s)
    want = fc.h_index(H, s, fmt, 16)
    got = index(torch, ctx, src, len(s), fmt, 16)
    print(f"{name}: {len(s) // 16} chunks, {got.candidates} candidates, {got.dropped} dropped, {got.rounds} rounds")
    assert len(s) // 16 > (20000 if name == "mix_mem1" else 200) and got.key() == want.key()
    assert got.candidates > (1000 if name == "mix_mem1" else 50)
    decode_with(torch, ctx, src, len(s), fmt, got.rows, data)


def test_state_of_the_context(torch, ctx):
    """the call leaves the "last decode" state alone, refuses while an asynchronous encode is unfinished, and a following encode
    and decode write what they write on a fresh context"""
    data = pc.data_of("alice")
    s = zlib.compress(data, 6)
    src, raw = dev(torch, s), dev(torch, data)
    dst = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    assert ctx.decode(src, len(s), dst, len(data), zz.Format.Zlib, 0) == len(data)
    before = (ctx.last_decode_path(), ctx.last_decode_stats())
    points, n = ctx.points_index(src, len(s), zz.Format.Zlib, 1000)
    assert n == len(data) and (ctx.last_decode_path(), ctx.last_decode_stats()) == before
    cap = zz.bound(len(data), zz.Format.Zlib, 1)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ctx.encode_async(raw, len(data), out, cap, zz.Format.Zlib, 1)
    e, m = u64(0), u64(0)
    assert zz.lib.zz_points_index_device(ctx._h, src.data_ptr(), len(s), 0, 1000, 1, None, 0, ctypes.byref(e), ctypes.byref(m), None) == zz.E_ARG
    w = ctx.finish()
    fresh = zz.Context(0)
    out2 = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    assert fresh.encode(raw, len(data), out2, cap, zz.Format.Zlib, 1) == w and torch.equal(out[:w], out2[:w])
    assert ctx.points_index(src, len(s), zz.Format.Zlib, 1000)[0].tolist() == points.tolist()
    back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    assert ctx.decode(out, w, back, len(data), zz.Format.Zlib) == len(data) and torch.equal(back, raw)
