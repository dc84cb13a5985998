"""zz_decode_points_ranges_device / Context.decode_points_ranges: reads of streams this library did not write, through a point
index with windows and sums. Every stream, index and sidecar goes through the bounds-checked CPU harness first
(tests/points_ranges_cases.py, tests/cxx/inflate_points_ranges_harness.cpp): the device run confirms what the harness found --
lengths, statuses, the bytes that were compressed, the segments decoded and the waves -- and on top of the harness's statuses the
independent rule holds everywhere: a read that reports ZZ_OK has exactly data[first : first + m].
(`out_off_by_one` on a zlib or gzip stream fails the whole call, not only the reads beside the row: the lied lengths no longer
fold to the trailer. test_points_ranges_cases_cpu.py's docstring has the reasoning.)
Needs a real MI355X: run with `-m gpu`."""
import ctypes
import zlib

import pytest

import points_cases as pc
import points_ranges_cases as prc
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
GUARD = prc.GUARD


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
    return prc.build_harness(tmp_path_factory.mktemp("points_ranges"))


@pytest.fixture(scope="module")
def sidecars(H):
    """name, spacing -> (rows, windows, sums) by the product's two host passes, held to the harness's builder, each made once"""
    memo = {}

    def get(name, spacing):
        if (name, spacing) not in memo:
            s, fmt, data = pc.case(name)
            points, n = zz.points_index_host(s, fmt, spacing)
            w, sm = zz.points_windows_host(s, points, fmt)
            rows = points.tolist()
            windows, sums = bytearray(w.numpy().tobytes()), [v & 0xFFFFFFFF for v in sm.tolist()]
            assert n == len(data) and prc.h_windows(H, s, fmt, rows) == (0, windows, sums), (name, spacing)
            memo[name, spacing] = (rows, windows, sums)
        return memo[name, spacing]
    return get


def dev(torch, b, lead=0):
    """the bytes on the device, `lead` bytes into their allocation (256-byte aligned plus lead)"""
    t = torch.zeros(lead + max(len(b), 1), dtype=torch.uint8, device="cuda")
    if b:
        t[lead: lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t[lead: lead + max(len(b), 1)]


def sidecar_dev(torch, rows, windows, sums, lead=0):
    points = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).cuda()
    w = dev(torch, bytes(windows), lead).reshape(len(rows) - 1, prc.WINDOW)
    sm = torch.tensor([v - (1 << 32) if v >> 31 else v for v in sums], dtype=torch.int32).cuda()
    return points, w, sm


class Got:
    pass


def run(torch, ctx, s, fmt, rows, windows, sums, reads, caps=None, src_lead=0, dst_lead=0, win_lead=0):
    """the call on the device: lens, status, the bytes of every ZZ_OK read, the call's code (from the statuses, or the refusal's),
    the stats. The GUARD bytes on both sides of every destination, and everything behind min(m, cap) of it, stay as they were."""
    caps = [n for _, n in reads] if caps is None else list(caps)
    src = dev(torch, s, src_lead)
    points, w, sm = sidecar_dev(torch, rows, windows, sums, win_lead)
    offs, at = [], dst_lead
    for c in caps:
        offs.append(at + GUARD)
        at += c + 2 * GUARD + ((-(c + 2 * GUARD)) % 8) + dst_lead
    whole = torch.full((at + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    dsts = [(whole.data_ptr() + o, c) for o, c in zip(offs, caps)]
    g = Got()
    try:
        g.lens, g.status = ctx.decode_points_ranges(src, len(s), points, w, sm, [f for f, _ in reads], [n for _, n in reads], dsts, caps, format=fmt)
        g.code = next((c for c in (prc.DATA, prc.UNSUPPORTED, prc.ARG, prc.NOSPACE) if c in g.status), prc.OK)
    except zz.ZzFlateError as e:
        g.lens, g.status, g.code = [None] * len(reads), None, e.code
    torch.cuda.synchronize()
    g.segments_decoded, g.waves = ctx.last_decode_points_ranges_stats()
    host = whole.cpu().numpy().tobytes()
    g.outs, g.untouched = [], True
    keep = bytearray(host)
    for r, (o, c) in enumerate(zip(offs, caps)):
        ok = g.status is not None and g.status[r] == prc.OK
        wrote = min(g.lens[r], c) if ok else (c if g.status is not None else 0)
        g.outs.append(host[o: o + g.lens[r]] if ok else None)
        keep[o: o + wrote] = b"\xEE" * wrote
    assert bytes(keep) == b"\xEE" * len(host), "bytes outside a destination (or behind a read's length) were written"
    g.untouched = host == b"\xEE" * len(host)
    return g


def same(g, want, what):
    """the device against the harness"""
    assert g.status == want.status and g.lens == want.lens and g.code == want.rc, what
    assert g.outs == want.outs, what
    assert (g.segments_decoded, g.waves) == (want.segments_decoded, want.waves), what


def ok_is_exact(g, reads, data, what):
    for (first, n), st, out in zip(reads, g.status, g.outs):
        if st == prc.OK:
            assert out == data[first: first + n], what


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_case_spacing_and_read(torch, ctx, H, sidecars, name):
    s, fmt, data = pc.case(name)
    for spacing in prc.SPACINGS:
        rows, windows, sums = sidecars(name, spacing)
        reads = prc.reads_for(rows)
        want = prc.h_reads(H, s, fmt, rows, windows, sums, reads)
        lens, status, outs, code, decoded = prc.expect(rows, data, reads)
        assert (want.lens, want.status, want.outs, want.rc, want.segments_decoded) == (lens, status, outs, code, decoded), (name, spacing)
        g = run(torch, ctx, s, fmt, rows, windows, sums, reads)
        print(f"{name} spacing {spacing}: {len(rows) - 1} segments, {len(reads)} reads, decoded {g.segments_decoded}, waves {g.waves}")
        same(g, want, (name, spacing))


def test_an_inverted_window_is_a_mismatch_not_wrong_bytes(torch, ctx, H, sidecars):
    s, fmt, data = pc.case("alice_mem1")
    rows, windows, sums = sidecars("alice_mem1", 1)
    ks = prc.aligned_segments(rows)
    assert len(ks) == 25
    for k in ks:
        reads = prc.damage_reads(rows, k)
        w = prc.inverted_slot(windows, rows, k)
        want = prc.h_reads(H, s, fmt, rows, w, sums, reads)
        assert want.win_copied[k] > 0 and want.status[0] == prc.DATA and want.status[1] == prc.OK
        g = run(torch, ctx, s, fmt, rows, w, sums, reads)
        same(g, want, k)
        ok_is_exact(g, reads, data, k)


def test_a_window_nobody_uses_may_hold_anything(torch, ctx, H, sidecars):
    s, fmt, data = pc.case("alice_flushes")
    rows, windows, sums = sidecars("alice_flushes", 1)
    honest = prc.h_reads(H, s, fmt, rows, windows, sums, [(0, len(data))])
    ks = prc.aligned_segments(rows)
    unused = [k for k in ks if honest.win_copied[k] == 0]
    assert (len(ks), len(unused)) == (49, 24)
    for k in ks:
        reads = prc.damage_reads(rows, k)
        w = prc.inverted_slot(windows, rows, k)
        want = prc.h_reads(H, s, fmt, rows, w, sums, reads)
        assert want.status[0] == (prc.OK if k in unused else prc.DATA)
        g = run(torch, ctx, s, fmt, rows, w, sums, reads)
        same(g, want, k)
        ok_is_exact(g, reads, data, k)


@pytest.mark.parametrize("name", prc.LIE_CASES)
def test_a_sums_entry_off_by_one(torch, ctx, H, sidecars, name):
    s, fmt, data = pc.case(name)
    rows, windows, sums = sidecars(name, 4096)
    reads = prc.reads_for(rows)
    for k in (0, len(sums) // 2, len(sums) - 1):
        sm = prc.sums_off_by_one(sums, k)
        want = prc.h_reads(H, s, fmt, rows, windows, sm, reads)
        g = run(torch, ctx, s, fmt, rows, windows, sm, reads)
        same(g, want, (name, k))
        ok_is_exact(g, reads, data, (name, k))
        if fmt == pc.RAW:
            assert prc.DATA in g.status and prc.OK in g.status
        else:
            assert set(g.status) == {prc.DATA} and g.code == prc.DATA and g.untouched and g.segments_decoded == 0


@pytest.mark.parametrize("name", prc.LIE_CASES)
def test_lying_indexes(torch, ctx, H, sidecars, name):
    s, fmt, data = pc.case(name)
    for spacing in prc.LIE_SPACINGS[name]:
        rows, windows, sums = sidecars(name, spacing)
        reads = prc.reads_for(rows)
        for kind in prc.SHAPE_LIES + prc.SEGMENT_LIES:
            r_, w_, s_ = prc.lied(rows, kind, s, windows, sums)
            want = prc.h_reads(H, s, fmt, r_, w_, s_, reads)
            g = run(torch, ctx, s, fmt, r_, w_, s_, reads)
            same(g, want, (name, spacing, kind))
            ok_is_exact(g, reads, data, (name, spacing, kind))
            if kind in prc.SHAPE_LIES or (kind == "out_off_by_one" and fmt != pc.RAW):
                assert set(g.status) == {prc.DATA} and g.code == prc.DATA and g.untouched and g.segments_decoded == 0, (name, spacing, kind)
            else:
                assert prc.OK in g.status and prc.DATA in g.status, (name, spacing, kind)


@pytest.mark.parametrize("name", ["alice_l6", "alice_gzip_header"])
def test_damaged_streams_with_honest_sidecars(torch, ctx, H, sidecars, name):
    s, fmt, data = pc.case(name)
    rows, windows, sums = sidecars(name, 4096)                # honest, made before the damage
    reads = prc.reads_for(rows)
    for bad in pc.flipped(s, count=25) + pc.truncated(s):
        assert pc.zlib_verdict(bad, fmt) is None
        want = prc.h_reads(H, bad, fmt, rows, windows, sums, reads)
        g = run(torch, ctx, bad, fmt, rows, windows, sums, reads)
        if want.rc == prc.UNSUPPORTED:                        # the flip asks for a preset dictionary: the call is refused
            assert g.code == prc.UNSUPPORTED and g.untouched
            continue
        same(g, want, len(bad))
        assert g.status[0] == prc.DATA, "the whole-stream read"
        ok_is_exact(g, reads, data, len(bad))


def test_a_distance_in_front_of_the_stream_is_refused_whatever_the_slot_holds(torch, ctx, H):
    raw, rows, windows, sums, data = prc.hand_made()
    reads = [(11, 1), (10, 3), (0, 10), (0, 13), (3, 2)]
    want = prc.h_reads(H, raw, pc.RAW, rows, windows, sums, reads)
    g = run(torch, ctx, raw, pc.RAW, rows, windows, sums, reads)
    same(g, want, "hand made")
    assert g.status == [prc.DATA, prc.DATA, prc.OK, prc.DATA, prc.OK] and g.outs[2] == data[:10] and g.outs[4] == data[3:5]


def test_only_what_is_touched_is_read(torch, ctx, H, sidecars):
    s, fmt, data = pc.case("mix_l6")
    rows, windows, sums = sidecars("mix_l6", 4096)
    L = len(data)
    reads = [(L // 2, 3000)]
    hit = prc.touched(rows, *reads[0])
    assert 0 < len(hit) < len(rows) - 1
    hl = pc.header_len(s, fmt)
    w, b = bytearray(windows), bytearray(s)
    for k in range(len(rows) - 1):
        if k in hit:
            continue
        w[k * prc.WINDOW: (k + 1) * prc.WINDOW] = b"\xFF" * prc.WINDOW
        lo, hi = hl + rows[k][0] // 8 + 1, hl + rows[k + 1][0] // 8          # strictly inside: not the bytes that hold a boundary bit
        if k + 1 not in hit and k - 1 not in hit and hi > lo:
            b[lo:hi] = b"\xFF" * (hi - lo)
    assert bytes(b) != s
    want = prc.h_reads(H, bytes(b), fmt, rows, w, sums, reads)
    g = run(torch, ctx, bytes(b), fmt, rows, w, sums, reads)
    same(g, want, "touched")
    assert g.status == [prc.OK] and g.outs == [data[L // 2: L // 2 + 3000]] and g.segments_decoded == len(hit)


def test_capacity_exact_and_one_short(torch, ctx, H, sidecars):
    s, fmt, data = pc.case("alice_mem1")
    rows, windows, sums = sidecars("alice_mem1", 4096)
    L = len(data)
    reads = [(100, 5000), (100, 5000), (L - 10, 100), (L - 10, 100), (7, 0)]
    caps = [5000, 4999, 10, 9, 0]
    want = prc.h_reads(H, s, fmt, rows, windows, sums, reads, caps)
    g = run(torch, ctx, s, fmt, rows, windows, sums, reads, caps)
    same(g, want, "caps")
    assert g.status == [prc.OK, prc.NOSPACE, prc.OK, prc.NOSPACE, prc.OK] and g.code == prc.NOSPACE
    assert g.lens == [5000, None, 10, None, 0] and g.outs[0] == data[100:5100] and g.outs[2] == data[L - 10:]


def test_argument_errors_before_anything_is_launched(torch, ctx, sidecars):
    s, fmt, data = pc.case("alice_mem1")
    rows, windows, sums = sidecars("alice_mem1", 4096)
    src = dev(torch, s)
    points, w, sm = sidecar_dev(torch, rows, windows, sums)
    dst = torch.full((1000,), 0xEE, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[0], [1000], [dst.data_ptr()], [1000]], dtype=torch.int64).cuda()
    lens = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    good = [ctx._h, src.data_ptr(), len(s), fmt, points.data_ptr(), len(rows), w.data_ptr(), sm.data_ptr(), 1, table[0].data_ptr(),
            table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(), lens.data_ptr(), status.data_ptr(), None]
    call = zz.lib.zz_decode_points_ranges_device
    for i in (0, 1, 4, 6, 7, 9, 10, 11, 12, 13):
        a = list(good)
        a[i] = None
        assert call(*a) == zz.E_ARG, i
    for i, v in ((5, 1), (5, (1 << 31) + 1), (8, 1 << 31), (3, 3), (3, -1)):
        a = list(good)
        a[i] = v
        assert call(*a) == zz.E_ARG, (i, v)
    # an unfinished asynchronous encode on the context
    raw = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    enc = torch.zeros(zz.bound(1000), dtype=torch.uint8, device="cuda")
    ctx.encode_async(raw, 1000, enc, enc.numel())
    assert call(*good) == zz.E_ARG
    ctx.finish()
    torch.cuda.synchronize()
    assert bool((dst == 0xEE).all()) and lens.item() == 7 and status.item() == 7, "a refused call wrote"
    assert call(*good) == 0 and lens.item() == 1000 and status.item() == 0
    assert dst.cpu().numpy().tobytes() == data[:1000]
    with pytest.raises(ValueError):                           # the sidecar must live on the context's device
        ctx.decode_points_ranges(src, len(s), points, w.cpu(), sm, [0], [10], [dst])
    with pytest.raises(ValueError):
        ctx.decode_points_ranges(src, len(s), points.cpu(), w, sm, [0], [10], [dst])


@pytest.mark.parametrize("lead", [1, 3, 7])
def test_misaligned_source_destination_and_windows(torch, ctx, H, sidecars, lead):
    for name in ("alice_mem1", "alice_l0", "alice_gzip_header"):
        s, fmt, data = pc.case(name)
        rows, windows, sums = sidecars(name, 4096)
        reads = prc.reads_for(rows)
        want = prc.h_reads(H, s, fmt, rows, windows, sums, reads)
        g = run(torch, ctx, s, fmt, rows, windows, sums, reads, src_lead=lead, dst_lead=8 - lead, win_lead=lead)
        same(g, want, (name, lead))
        ok_is_exact(g, reads, data, (name, lead))


def test_the_encoders_and_the_other_decoders_last_state_is_left_alone(torch, ctx, H, sidecars):
    import gzip
    d = pc.data_of("alice")
    src = dev(torch, d)
    cap = zz.bound(len(d), 0, 2, 4096)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, len(d), dst, cap, 0, 2, 4096)
    out = torch.zeros(len(d), dtype=torch.uint8, device="cuda")
    assert ctx.decode(dst, w, out, len(d), 0, 4096) == len(d)
    mcap = zz.members_bound(len(d))
    mdst = torch.zeros(mcap, dtype=torch.uint8, device="cuda")
    mw = ctx.encode_members(src, len(d), mdst, mcap, level=1)
    index = ctx.members_index(mdst, mw)
    ctx.decode_members_ranges(mdst, mw, index, [5], [70000], [out])
    w2 = ctx.encode(src, len(d), dst, cap, 0, 2, 4096)
    assert w2 == w
    before = (ctx.verify_last(), ctx.packet_index().cpu().tolist(), ctx.last_decode_path(), ctx.last_decode_stats(),
              ctx.last_decode_members_ranges_stats(), ctx.last_decode_members_stats(), ctx.last_decode_ranges_stats())
    assert before[4][0] >= 2
    s, fmt, data = pc.case("alice_mem1")
    rows, windows, sums = sidecars("alice_mem1", 4096)
    reads = [(1000, 50000)]
    g = run(torch, ctx, s, fmt, rows, windows, sums, reads)
    assert g.status == [prc.OK] and g.outs == [data[1000:51000]] and g.segments_decoded >= 2
    after = (ctx.verify_last(), ctx.packet_index().cpu().tolist(), ctx.last_decode_path(), ctx.last_decode_stats(),
             ctx.last_decode_members_ranges_stats(), ctx.last_decode_members_stats(), ctx.last_decode_ranges_stats())
    assert after == before
    assert gzip.decompress(mdst[:mw].cpu().numpy().tobytes()) == d


def test_member_reads_and_point_reads_take_turns_on_one_context(torch, sidecars):
    """The two calls share one workspace. A member call with an index of a few entries and four reads, a point call whose index
    and reads are more and whose rooms are more (every buffer sized by entries, reads, a wave's units or a wave's bytes grows
    between the calls), the member call again: bytes, lengths, statuses and codes are those of fresh contexts, and the member
    reads' stats outlive the point call."""
    d = pc.data_of("alice")
    src = dev(torch, d)
    mcap = zz.members_bound(len(d))
    mdst = torch.zeros(mcap, dtype=torch.uint8, device="cuda")
    mw = zz.Context(0).encode_members(src, len(d), mdst, mcap, level=1)
    index = zz.Context(0).members_index(mdst, mw)
    mreads, mcaps = [(10, 100), (100, 50), (len(d) - 20, 100), (5000, 300)], [100, 50, 100, 299]     # (the first and the last member)
    s, fmt, data = pc.case("alice_mem1")
    rows, windows, sums = sidecars("alice_mem1", 4096)
    preads = prc.reads_for(rows)
    assert len(rows) > index.shape[0] and len(preads) > len(mreads) and len(prc.touched(rows, 0, len(data))) > index.shape[0] - 1

    def members(c):
        outs = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _, n in mreads]
        lens, status = c.decode_members_ranges(mdst, mw, index, [f for f, _ in mreads], [n for _, n in mreads], outs, mcaps)
        code = next((v for v in (prc.DATA, prc.UNSUPPORTED, prc.ARG, prc.NOSPACE) if v in status), prc.OK)
        return lens, status, code, [o.cpu().numpy().tobytes() for o in outs], c.last_decode_members_ranges_stats()

    def points(c):
        g = run(torch, c, s, fmt, rows, windows, sums, preads)
        return g.lens, g.status, g.code, g.outs, (g.segments_decoded, g.waves)

    fresh_m, fresh_p = members(zz.Context(0)), points(zz.Context(0))
    assert fresh_m[:3] == ([100, 50, 20, None], [prc.OK, prc.OK, prc.OK, prc.NOSPACE], prc.NOSPACE)
    assert [o[:m] for o, m, (f, _) in zip(fresh_m[3], fresh_m[0], mreads) if m is not None] == [d[f: f + m] for (f, _), m in zip(mreads, fresh_m[0]) if m is not None]
    assert fresh_m[4][0] >= 2 and fresh_p[4][0] > fresh_m[4][0] and prc.OK in fresh_p[1]
    one = zz.Context(0)
    assert members(one) == fresh_m
    assert points(one) == fresh_p
    assert one.last_decode_members_ranges_stats() == fresh_m[4]
    assert members(one) == fresh_m
    assert one.last_decode_points_ranges_stats() == fresh_p[4]


@pytest.fixture(scope="module")
def big():
    """96 MiB across a real wave edge (64 MiB of rooms): the periodic pattern with alice29.txt spliced in every 8 MiB, zlib level 1"""
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


def test_ninety_six_mib_across_a_wave_edge(torch, ctx, big):
    s, data, points = big
    rows = points.tolist()
    windows, sums = zz.points_windows_host(s, points, pc.ZLIB)
    L = len(data)
    assert L > prc.STAGE and len(rows) > 3 and prc.waves_of(rows, [(0, L)]) >= 2
    src = dev(torch, s)
    dst = torch.full((L + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    lens, status = ctx.decode_points_ranges(src, len(s), points.cuda(), windows.cuda(), sums.cuda(), [0], [L], [(dst.data_ptr(), L)], format=pc.ZLIB)
    assert (lens, status) == ([L], [0])
    expect = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    assert bool(torch.equal(dst[:L], expect)) and bool((dst[L:] == 0xEE).all())
    decoded, waves = ctx.last_decode_points_ranges_stats()
    print(f"96 MiB: {len(rows) - 1} segments, decoded {decoded}, waves {waves}")
    assert decoded == len(prc.touched(rows, 0, L)) and waves == prc.waves_of(rows, [(0, L)]) >= 2
    # the same stream through a one-segment index: a room above the stage, nothing decoded
    one = points[[0, -1]].contiguous()
    w1, s1 = zz.points_windows_host(s, one, pc.ZLIB)
    dst.fill_(0xEE)
    lens, status = ctx.decode_points_ranges(src, len(s), one.cuda(), w1.cuda(), s1.cuda(), [0, 5], [L, 10], [(dst.data_ptr(), L), (dst.data_ptr(), 10)],
                                            format=pc.ZLIB)
    assert (lens, status) == ([None, None], [prc.UNSUPPORTED, prc.UNSUPPORTED])
    assert ctx.last_decode_points_ranges_stats() == (0, 1) and bool((dst == 0xEE).all())


def test_the_single_read_wrapper(torch, ctx, sidecars):
    s, fmt, data = pc.case("mix_l6")
    rows, windows, sums = sidecars("mix_l6", 32768)
    src = dev(torch, s)
    points, w, sm = sidecar_dev(torch, rows, windows, sums)
    L = len(data)
    for first, n in ((0, 100), (L // 2, 70000), (L - 5, 100)):
        dst = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        m = ctx.decode_points_range(src, len(s), points, w, sm, first, n, dst[:n], format=fmt)
        assert m == min(n, L - first) and dst[:m].cpu().numpy().tobytes() == data[first: first + m]
        assert bool((dst[m:] == 0xEE).all())
    with pytest.raises(zz.ZzFlateError) as e:
        ctx.decode_points_range(src, len(s), points, w, sm, L + 1, 10, torch.zeros(10, dtype=torch.uint8, device="cuda"), format=fmt)
    assert e.value.code == zz.E_ARG
    with pytest.raises(zz.ZzFlateError) as e:
        ctx.decode_points_range(src, len(s), points, w, sm, 0, 100, torch.zeros(100, dtype=torch.uint8, device="cuda"), cap=99, format=fmt)
    assert e.value.code == zz.E_NOSPACE
