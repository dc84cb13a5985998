"""zz_points_windows_device / Context.points_windows / Context.open_found: the window sidecar of a point index built on the device.
The list is tests/points_windows_cases.py's, which test_points_windows_cpu.py has sent through the bounds-checked CPU harness
(tests/cxx/points_windows_harness.cpp) case by case; the yardstick is zz_points_windows_host's two tensors, whole, zeros included,
and the bytes that were compressed. Windows, sums and the destination lie between guard bytes in every call made here through the
C ABI. Nothing here provokes a fault: refused inputs are refused by checks.
Needs a real MI355X: run with `-m gpu`."""
import ctypes

import pytest

import points_cases as pc
import points_ranges_cases as prc
import points_windows_cases as pw
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


@pytest.fixture(scope="module")
def on_device(torch):
    """name -> the stream on the device; (name, spacing) -> the host builder's sidecar on the device; each moved once"""
    memo = {}

    def get(name, spacing=None):
        if (name, spacing) not in memo:
            if spacing is None:
                memo[name, None] = dev(torch, pc.case(name)[0])
            else:
                w, s = pw.host_sidecar(name, spacing)
                memo[name, spacing] = (w.cuda(), s.cuda())
        return memo[name, spacing]
    return get


def dev(torch, b):
    t = torch.zeros(max(len(b), 1), dtype=torch.uint8, device="cuda")
    if b:
        t[: len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t


class Got:
    pass


def build(torch, ctx, src, src_len, fmt, points, fine=None, stage=0, cap=None):
    """the call through the C ABI with windows, sums and the destination (cap: None, or its capacity) between GUARD bytes of one
    allocation filled with 0xEE; the guards must come back untouched whatever the call answers"""
    segments = points.shape[0] - 1
    sizes = [segments * pw.WINDOW, segments * 4, 0 if cap is None else cap]
    offs, at = [], GUARD
    for n in sizes:
        offs.append(at)
        at += n + GUARD + (-n) % 8
    whole = torch.full((at,), 0xEE, dtype=torch.uint8, device="cuda")
    base = whole.data_ptr()
    g = Got()
    g.code = zz.lib.zz_points_windows_device(ctx._h, src.data_ptr(), src_len, int(pw.FMT[fmt]), points.data_ptr(), points.shape[0],
                                             None if fine is None else fine.data_ptr(), 0 if fine is None else fine.shape[0],
                                             base + offs[0], base + offs[1], None if cap is None else base + offs[2], cap or 0, stage,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g.windows = whole[offs[0]: offs[0] + sizes[0]].reshape(segments, pw.WINDOW)
    g.sums = whole[offs[1]: offs[1] + sizes[1]].view(torch.int32)
    g.out = whole[offs[2]: offs[2] + sizes[2]]
    keep = whole.clone()
    for o, n in zip(offs, sizes):
        keep[o: o + n] = 0xEE
    assert bool((keep == 0xEE).all()), "bytes outside windows, sums or the destination were written"
    g.untouched = bool((whole == 0xEE).all())
    g.stats = ctx.last_points_windows_stats()
    return g


def check_honest(torch, ctx, on_device, c, with_dst=False):
    name, spacing, fine, stage = c
    s, fmt, data = pc.case(name)
    plan = pw.plan_of(c, with_dst)
    g = build(torch, ctx, on_device(name), len(s), fmt, pw.rows_of(name, spacing), pw.rows_of(name, 1) if fine else None, stage,
              len(data) if with_dst else None)
    assert g.code == plan.code, pw.case_id(c)
    if g.code != pw.OK:
        return
    w, sm = on_device(name, spacing)
    assert torch.equal(g.sums, sm), pw.case_id(c)
    assert torch.equal(g.windows, w), pw.case_id(c)
    assert g.stats[0] == plan.batches, pw.case_id(c)
    if with_dst:
        assert g.out.cpu().numpy().tobytes() == data, pw.case_id(c)


@pytest.mark.parametrize("name", pw.STREAMS)
def test_the_device_makes_the_host_builders_sidecar(torch, ctx, on_device, name):
    for c in pw.cases():
        if c[0] == name:
            check_honest(torch, ctx, on_device, c)


@pytest.mark.parametrize("name", pw.STREAMS)
def test_with_a_destination_the_stream_is_left_there(torch, ctx, on_device, name):
    for c in pw.cases():
        if c[0] == name and c[1] in (4096, 1 << 40) and c[3] in (0, 40000, pw.TINY_STAGE):
            check_honest(torch, ctx, on_device, c, with_dst=True)


@pytest.mark.parametrize("name", ["alice_mem1", "mix_l6", "mix_l9_raw"])
def test_the_devices_sidecar_serves_the_reads(torch, ctx, on_device, name):
    s, fmt, data = pc.case(name)
    points = pw.rows_of(name, 4096)
    dense = pw.rows_of(name, 1)
    windows, sums = ctx.points_windows(on_device(name), len(s), points, pw.FMT[fmt], fine_points=dense, stage_bytes=pw.longest(pw.as_lists(dense)))
    assert windows.dtype == torch.uint8 and tuple(windows.shape) == (points.shape[0] - 1, pw.WINDOW) and windows.is_cuda
    assert sums.dtype == torch.int32 and tuple(sums.shape) == (points.shape[0] - 1,) and sums.is_cuda
    w, sm = on_device(name, 4096)
    assert torch.equal(windows, w) and torch.equal(sums, sm)
    reads = prc.reads_for(pw.as_lists(points))
    outs = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _, n in reads]
    lens, status = ctx.decode_points_ranges(on_device(name), len(s), points.cuda(), windows, sums, [f for f, _ in reads], [n for _, n in reads],
                                            outs, format=pw.FMT[fmt])
    want_lens, want_status, want_outs, _, _ = prc.expect(pw.as_lists(points), data, reads)
    assert status == want_status
    for r, st in enumerate(status):
        if st == pw.OK:
            assert lens[r] == want_lens[r] and outs[r][: lens[r]].cpu().numpy().tobytes() == want_outs[r], reads[r]
    assert pw.OK in status


@pytest.mark.parametrize("name", ["alice_l6", "mix_l6", "alice_raw"])
def test_open_found(torch, ctx, on_device, name):
    s, fmt, data = pc.case(name)
    spacing = 32768
    src = on_device(name)
    dense, n = ctx.points_index(src, len(s), pw.FMT[fmt], 4096, 1)
    want_rows = zz.points_thin(dense, spacing)
    want_w, want_s = zz.points_windows_host(s, want_rows, pw.FMT[fmt])
    for with_dst in (False, True):
        dst = torch.full((len(data) + 64,), 0xEE, dtype=torch.uint8, device="cuda") if with_dst else None
        points, windows, sums, length = ctx.open_found(src, len(s), pw.FMT[fmt], 4096, spacing, dst, len(data) if with_dst else None)
        assert length == n == len(data)
        assert points.is_cuda and torch.equal(points.cpu(), want_rows)
        assert torch.equal(windows.cpu(), want_w) and torch.equal(sums.cpu(), want_s)
        first, m = len(data) // 2 - 100, 4096
        out = torch.zeros(m, dtype=torch.uint8, device="cuda")
        lens, status = ctx.decode_points_ranges(src, len(s), points, windows, sums, [first], [m], [out], format=pw.FMT[fmt])
        assert status == [0] and lens == [m] and out.cpu().numpy().tobytes() == data[first: first + m]
        if with_dst:
            host = dst.cpu().numpy().tobytes()
            assert host[: len(data)] == data and host[len(data):] == b"\xEE" * 64


def host_code(s, fmt, rows):
    segments = max(len(rows) - 1, 1)
    win = (ctypes.c_uint8 * (segments * pw.WINDOW))()
    sums = (ctypes.c_uint32 * segments)()
    return zz.lib.zz_points_windows_host(s, len(s), fmt, pc.flat(rows), len(rows), win, sums)


def honest_again(torch, ctx, on_device):
    """the context serves a correct call after a refused one"""
    check_honest(torch, ctx, on_device, ("alice_mem1", 4096, True, 40000))


@pytest.mark.parametrize("name", prc.LIE_CASES)
def test_lying_indexes_get_the_host_builders_verdict(torch, ctx, on_device, name):
    s, fmt, _ = pc.case(name)
    for spacing in prc.LIE_SPACINGS[name]:
        rows = pw.as_lists(pw.rows_of(name, spacing))
        for kind in prc.SHAPE_LIES + prc.SEGMENT_LIES:
            lied = pc.lie(rows, kind, len(s))
            want = host_code(s, fmt, lied)
            assert want == pw.DATA
            g = build(torch, ctx, on_device(name), len(s), fmt, torch.tensor(lied, dtype=torch.int64))
            assert g.code == want, (name, spacing, kind)
    honest_again(torch, ctx, on_device)


@pytest.mark.parametrize("name", ["alice_l6", "alice_gzip_header", "alice_raw"])
def test_damaged_streams_get_the_host_builders_verdict(torch, ctx, on_device, name):
    s, fmt, _ = pc.case(name)
    points = pw.rows_of(name, 4096)
    rows = pw.as_lists(points)
    seen = set()
    for bad in pc.flipped(s, count=25) + pc.truncated(s) + (pw.trailer_damaged(s, fmt) if fmt != pc.RAW else []):
        want = host_code(bad, fmt, rows)
        seen.add(want)
        g = build(torch, ctx, dev(torch, bad), len(bad), fmt, points, cap=rows[-1][1])
        assert g.code == want
    assert pw.DATA in seen
    honest_again(torch, ctx, on_device)


def test_refusals_through_the_abi(torch, ctx, on_device):
    # trailer-only damage: zlib and gzip
    for name in ("alice_l6", "mix_l6"):
        s, fmt, data = pc.case(name)
        for bad in pw.trailer_damaged(s, fmt):
            assert pc.zlib_verdict(bad, fmt) is None
            g = build(torch, ctx, dev(torch, bad), len(bad), fmt, pw.rows_of(name, 32768), pw.rows_of(name, 1), pw.longest(pw.as_lists(pw.rows_of(name, 1))))
            assert g.code == pw.DATA and b"trailer" in zz.lib.zz_last_error()
    # a stage one byte short, and a destination one byte short (nothing is written)
    name = "alice_mem1"
    s, fmt, data = pc.case(name)
    points, dense = pw.rows_of(name, 4096), pw.rows_of(name, 1)
    need = pw.longest(pw.as_lists(dense))
    assert build(torch, ctx, on_device(name), len(s), fmt, points, dense, need).code == pw.OK
    assert build(torch, ctx, on_device(name), len(s), fmt, points, dense, need - 1).code == pw.UNSUPPORTED
    g = build(torch, ctx, on_device(name), len(s), fmt, points, dense, 0, cap=len(data) - 1)
    assert g.code == pw.NOSPACE and g.untouched
    # the planted far distance in a batch whose base is 10
    raw, rows, _, _, _ = prc.hand_made()
    for stage, cap in ((10, None), (0, None), (10, 13)):
        g = build(torch, ctx, dev(torch, raw), len(raw), pc.RAW, torch.tensor(rows, dtype=torch.int64), None, stage, cap)
        assert g.code == pw.DATA, (stage, cap)
    # a preset dictionary
    s, fmt, _ = pc.case("alice_l6")
    fdict = bytearray(s)
    fdict[1] = (fdict[1] & 0xC0) | 0x20                                  # FLEVEL kept, FDICT set, FCHECK made to fit
    fdict[1] |= (31 - (fdict[0] * 256 + fdict[1]) % 31) % 31
    assert fdict[1] & 0x20 and (fdict[0] * 256 + fdict[1]) % 31 == 0
    assert build(torch, ctx, dev(torch, bytes(fdict)), len(s), fmt, pw.rows_of("alice_l6", 32768)).code == pw.UNSUPPORTED
    honest_again(torch, ctx, on_device)


def test_the_decode_calls_state_is_left_alone(torch, ctx, on_device):
    name = "alice_mem1"
    s, fmt, data = pc.case(name)
    back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    assert ctx.decode_points(on_device(name), len(s), back, len(data), pw.rows_of(name, 4096), pw.FMT[fmt]) == len(data)
    path, stats = ctx.last_decode_path(), ctx.last_decode_stats()
    assert path == zz.DECODE_POINTS
    ranges = ctx.last_decode_points_ranges_stats()
    check_honest(torch, ctx, on_device, (name, 4096, True, 40000))
    assert ctx.last_points_windows_stats()[0] >= 3
    assert (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_points_ranges_stats()) == (path, stats, ranges)
    with pytest.raises(zz.ZzFlateError):
        ctx.points_windows(on_device(name), len(s), pw.rows_of(name, 4096), pw.FMT[fmt], stage_bytes=100)
    assert (ctx.last_decode_path(), ctx.last_decode_stats()) == (path, stats)
