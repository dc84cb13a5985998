"""zz_decode_points_device / Context.decode_points: streams this library did not write, decoded in parallel from a point index.
Every stream and index goes through the bounds-checked CPU harness first (tests/points_cases.py, tests/cxx/inflate_points_harness.cpp):
the device run confirms what the harness found -- the bytes that were compressed, the path, the pending bytes and the rounds.

The rounds: the harness runs them synchronously (a round reads what the round before left). k_inflate_resolve, reused as it is,
lets a byte adopt "the old pointer or this round's: both lead there", so on the device a byte whose target was already served in
the same round jumps further, and the device can finish in FEWER rounds than the harness, never in more; which of the two it
reads is a matter of timing. A byte whose target is pending cannot be final in round 1 under either rule, so up to two rounds the
count is determinate. check_rounds asserts exactly that: equal up to 2, else 2 <= device <= harness. Measured on an MI355X:
equal in every case of the list but two, both at spacing 1 with several segments inside one tile -- alice_mem1 (242 segments)
4 rounds for the harness's 6, mix_mem1 (1,945 segments) 7 for 9. The pending bytes are equal everywhere.
Needs a real MI355X: run with `-m gpu`."""
import ctypes
import zlib

import pytest

import points_cases as pc
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
GUARD = 64


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
    return pc.build_harness(tmp_path_factory.mktemp("points"))


def dev(torch, b, lead=0):
    """the bytes on the device, `lead` bytes into their allocation (256-byte aligned plus lead)"""
    t = torch.zeros(lead + max(len(b), 1), dtype=torch.uint8, device="cuda")
    if b:
        t[lead: lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t, t[lead:]


def run(torch, ctx, s, fmt, points, cap, src_lead=0, dst_lead=0):
    """(code, bytes, path, (pending, rounds)); the guard bytes behind `cap` and in front of the destination stay as they were"""
    _keep, src = dev(torch, s, src_lead)
    whole = torch.full((dst_lead + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = whole[dst_lead:]
    try:
        n, code = ctx.decode_points(src.data_ptr(), len(s), dst.data_ptr(), cap, points, fmt), 0
    except zz.ZzFlateError as e:
        n, code = 0, e.code
    torch.cuda.synchronize()
    host = whole.cpu().numpy().tobytes()
    assert host[:dst_lead] == b"\xEE" * dst_lead and host[dst_lead + cap:] == b"\xEE" * GUARD, "bytes outside the destination were written"
    return code, host[dst_lead: dst_lead + n], ctx.last_decode_path(), ctx.last_decode_stats()


def check_rounds(rounds, want, what):
    if want <= 2:
        assert rounds == want, what
    else:
        assert 2 <= rounds <= want, what


def tensor(torch, rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_case_at_every_spacing(torch, ctx, H, name):
    s, fmt, data = pc.case(name)
    for spacing in pc.SPACINGS:
        points, n = zz.points_index_host(s, fmt, spacing)
        rows = points.tolist()
        want = pc.h_decode(H, s, fmt, rows, len(data))
        assert (want.rc, want.path, n) == (0, pc.PATH_POINTS, len(data)) and want.out == data
        code, got, path, (pending, rounds) = run(torch, ctx, s, fmt, points, len(data))
        print(f"{name} spacing {spacing}: {len(rows) - 1} segments, pending {pending} (harness {want.pending}), "
              f"rounds {rounds} (harness {want.rounds})")
        assert code == 0 and got == data, (name, spacing)
        assert path == zz.DECODE_POINTS
        assert pending == want.pending, (name, spacing)
        check_rounds(rounds, want.rounds, (name, spacing))


@pytest.mark.parametrize("name, spacing", [("alice_mem1", 4096), ("mix_mem1", 32768)])
def test_lying_indexes_give_the_bytes_on_the_serial_path(torch, ctx, H, name, spacing):
    s, fmt, data = pc.case(name)
    rows = zz.points_index_host(s, fmt, spacing)[0].tolist()
    sn = len(s) - pc.header_len(s, fmt) - pc.TRAILER[fmt]
    for kind in pc.LIES:
        bad = pc.lie(rows, kind, sn)
        want = pc.h_decode(H, s, fmt, bad, len(data))
        assert (want.rc, want.path) == (0, pc.PATH_SERIAL) and want.out == data
        code, got, path, stats = run(torch, ctx, s, fmt, tensor(torch, bad), len(data))
        assert code == 0 and got == data, kind
        assert path == zz.DECODE_SERIAL and stats == (0, 0), kind


@pytest.mark.parametrize("name", ["alice_l6", "alice_gzip_header"])
def test_damaged_streams(torch, ctx, H, name):
    s, fmt, data = pc.case(name)
    points = zz.points_index_host(s, fmt, 4096)[0]             # honest, made before the damage
    for bad in pc.flipped(s, 25) + pc.truncated(s):
        assert pc.zlib_verdict(bad, fmt) is None
        want = pc.h_decode(H, bad, fmt, points.tolist(), len(data) + 100)
        assert want.rc == zz.E_DATA
        code, got, _path, _stats = run(torch, ctx, bad, fmt, points, len(data) + 100)
        assert code == zz.E_DATA and got == b""


def test_capacity_exact_and_one_short(torch, ctx, H):
    for name in ("alice_mem1", "alice_l0", "one_zlib"):
        s, fmt, data = pc.case(name)
        points = zz.points_index_host(s, fmt, 4096)[0]
        assert pc.h_decode(H, s, fmt, points.tolist(), len(data)).path == pc.PATH_POINTS
        code, got, path, _ = run(torch, ctx, s, fmt, points, len(data))
        assert (code, path) == (0, zz.DECODE_POINTS) and got == data
        assert pc.h_decode(H, s, fmt, points.tolist(), len(data) - 1).rc == zz.E_NOSPACE
        code, got, _path, _ = run(torch, ctx, s, fmt, points, len(data) - 1)     # (run() checks the guard bytes)
        assert code == zz.E_NOSPACE


def test_argument_errors_before_anything_is_launched(torch, ctx):
    s, fmt, data = pc.case("alice_l6")
    _keep, src = dev(torch, s)
    dst = torch.full((len(data),), 0xEE, dtype=torch.uint8, device="cuda")
    rows = (ctypes.c_uint64 * 4)(0, 0, 8 * (len(s) - 6), len(data))
    out = ctypes.c_uint64(7)
    L, h = zz.lib, ctx._h
    call = lambda *a: L.zz_decode_points_device(*a)
    sp, dp, op = src.data_ptr(), dst.data_ptr(), ctypes.byref(out)
    assert call(None, sp, len(s), dp, len(data), op, fmt, rows, 2, None) == zz.E_ARG
    assert call(h, None, len(s), dp, len(data), op, fmt, rows, 2, None) == zz.E_ARG
    assert call(h, sp, len(s), dp, len(data), None, fmt, rows, 2, None) == zz.E_ARG
    assert call(h, sp, len(s), dp, len(data), op, fmt, None, 2, None) == zz.E_ARG
    assert call(h, sp, len(s), dp, len(data), op, fmt, rows, 1, None) == zz.E_ARG
    assert call(h, sp, len(s), dp, len(data), op, 3, rows, 2, None) == zz.E_ARG
    assert call(h, sp, len(s), dp, len(data), op, -1, rows, 2, None) == zz.E_ARG
    # an unfinished asynchronous encode on the context
    raw = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    enc = torch.zeros(zz.bound(1000), dtype=torch.uint8, device="cuda")
    ctx.encode_async(raw, 1000, enc, enc.numel())
    assert call(h, sp, len(s), dp, len(data), op, fmt, rows, 2, None) == zz.E_ARG
    ctx.finish()
    torch.cuda.synchronize()
    assert bool((dst == 0xEE).all()), "a refused call wrote to the destination"
    with pytest.raises(ValueError):
        ctx.decode_points(src, len(s), dst, len(data), zz.points_index_host(s, fmt)[0].cuda(), fmt)


@pytest.mark.parametrize("lead", [1, 3, 7])
def test_misaligned_source_and_destination(torch, ctx, H, lead):
    for name in ("alice_mem1", "alice_l0", "alice_gzip_header"):
        s, fmt, data = pc.case(name)
        points = zz.points_index_host(s, fmt, 4096)[0]
        assert pc.h_decode(H, s, fmt, points.tolist(), len(data)).out == data
        code, got, path, _ = run(torch, ctx, s, fmt, points, len(data), src_lead=lead, dst_lead=8 - lead)
        assert (code, path) == (0, zz.DECODE_POINTS) and got == data


def test_the_encoders_last_call_state_is_left_alone(torch, ctx, H):
    d = pc.data_of("alice")
    _k, src = dev(torch, d)
    cap = zz.bound(len(d), 0, 2, 4096)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, len(d), dst, cap, 0, 2, 4096)
    before = (ctx.verify_last(), ctx.packet_index().cpu().tolist())
    s, fmt, data = pc.case("alice_mem1")
    points = zz.points_index_host(s, fmt, 4096)[0]
    assert pc.h_decode(H, s, fmt, points.tolist(), len(data)).out == data
    code, got, path, _ = run(torch, ctx, s, fmt, points, len(data))
    assert (code, path) == (0, zz.DECODE_POINTS) and got == data
    assert (ctx.verify_last(), ctx.packet_index().cpu().tolist()) == before
    # and a decode through the packet index behind it reports its own path and stats again
    out = torch.zeros(len(d), dtype=torch.uint8, device="cuda")
    assert ctx.decode(dst, w, out, len(d), 0, 4096) == len(d)
    assert ctx.last_decode_path() == zz.DECODE_DISCOVERED


@pytest.fixture(scope="module")
def big():
    """96 MiB across a real batch edge (64 MiB): the periodic pattern with alice29.txt spliced in every 8 MiB, zlib level 1"""
    alice, period = pc.data_of("alice"), pc.data_of("periodic")[:1000]
    parts = []
    stretch = (period * (8 * 1048576 // 1000 + 1))[: 8 * 1048576 - len(alice)]
    for _ in range(12):
        parts += [stretch, alice]
    data = b"".join(parts)
    s = zlib.compress(data, 1)
    points, n = zz.points_index_host(s, pc.ZLIB)
    assert n == len(data) == 96 * 1048576
    return s, data, points


def test_ninety_six_mib_across_a_batch_edge(torch, ctx, H, big):
    s, data, points = big
    rows = points.tolist()
    assert rows[-1][1] > pc.BATCH and len(rows) > 3
    want = pc.h_decode(H, s, pc.ZLIB, rows, len(data))
    assert (want.rc, want.path) == (0, pc.PATH_POINTS) and want.batches >= 2 and want.out == data
    _keep, src = dev(torch, s)
    dst = torch.full((len(data) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    assert ctx.decode_points(src, len(s), dst, len(data), points, pc.ZLIB) == len(data)
    assert ctx.last_decode_path() == zz.DECODE_POINTS
    expect = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    assert bool(torch.equal(dst[: len(data)], expect)) and bool((dst[len(data):] == 0xEE).all())
    pending, rounds = ctx.last_decode_stats()
    print(f"96 MiB: {len(rows) - 1} segments, pending {pending} (harness {want.pending}), rounds {rounds} (harness {want.rounds})")
    assert pending == want.pending
    check_rounds(rounds, want.rounds, "96 MiB")
