"""The checksum partials, their folds and the packet join at their round edges (tests/join_cases.py; the guards that need no GPU
are in tests/test_join_cases_cpu.py). Every encoder form that owns a partial or a fold runs over the part of the list that
reaches it: its stream equals oracle.encode_packets byte for byte, and its trailer -- compared on its own -- is the one Python's
zlib computes from the input. Shard partials equal zlib's value for the shard's bytes and fold to the whole trailer. The same
streams go back through every decode path, and a trailer that is off by one is E_DATA on each of them with nothing written
outside the destination. Every expectation is exact. Needs a real MI355X: run with `-m gpu`."""
import ctypes
import zlib

import pytest

import join_cases as jc
import members_write_cases as mw
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
GUARD = 64
SMALL = 400000                          # cases up to this many bytes also take the serial and the batch decoders


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    c = zz.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def xctx(torch):
    c = zz.Context(0)
    c.set_extended_levels(True)
    yield c
    c.close()


_want = {}


def want(oracle, c, fmt, lvl, warm=0):
    """the oracle's stream, computed once for the tests that share it (the largest inputs are not kept)"""
    key = (c, fmt, lvl, warm)
    if key in _want:
        return _want[key]
    s = oracle.encode_packets(jc.data(c), fmt, lvl, c.P, warm)
    if c.n <= 4 * SMALL:
        _want[key] = s
    return s


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def encode(torch, ctx, src, n, fmt, lvl, P):
    """(stream as a device tensor, its bytes): the destination has the bound's bytes and GUARD bytes of 0xA5 behind them"""
    cap = zz.bound(n, fmt, min(lvl, 3), P)
    dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, n, dst, cap, fmt, lvl, P)
    assert w <= cap and bool((dst[cap:] == 0xA5).all())
    return dst[:w], dst[:w].cpu().numpy().tobytes()


def check_stream(got, expect, d, fmt, what):
    """byte for byte the oracle's, and -- independently -- the trailer by zlib"""
    t = jc.trailer(d, fmt)
    assert got[len(got) - len(t):] == t, ("trailer", what, got[len(got) - len(t):].hex(), t.hex())
    assert got == expect, ("stream", what, len(got), len(expect))


def run_cases(torch, ctx, oracle, cases, fmt, lvl, warm=0):
    for c in cases:
        d = jc.data(c)
        _, got = encode(torch, ctx, dev(torch, d), c.n, fmt, lvl, c.P)
        check_stream(got, want(oracle, c, fmt, lvl, warm), d, fmt, (jc.case_id(c), fmt, lvl, warm))


def short_rounds(lvl, most=2049):
    return [c for c in jc.group("round", lvl) if jc.npk(c) <= most]


# ---- encode ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grp", ["len", "mod", "part", "crc", "round"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_encode(torch, ctx, oracle, lvl, fmt, grp):
    """Context.encode: k_encode_l0's coop_copy_adler, wave_adler_part in k_encode_l1p, the sums fused into the level-2 helper
    pass, crc32_packets_run on both of its paths; k_cks_reduce, k_scan_sizes and k_compact past their rounds and grids"""
    cases = jc.group(grp, lvl)
    assert cases
    run_cases(torch, ctx, oracle, cases, fmt, lvl)


@pytest.mark.parametrize("warm", [258, 32768])
@pytest.mark.parametrize("lvl", [1, 2])
def test_warm_window(torch, oracle, lvl, warm):
    """the warm-window kernels: k_encode_l1pw sums a packet with wave_adler on one wavefront"""
    c = zz.Context(0)
    c.set_warm_window(warm)
    try:
        run_cases(torch, c, oracle, jc.group("len", lvl) + jc.group("mod", lvl) + jc.group("part", lvl) + short_rounds(lvl), 0, lvl, warm)
    finally:
        c.close()


@pytest.mark.parametrize("lvl", [4, 5, 6])
def test_extended_levels(torch, xctx, oracle, lvl):
    """levels 4..6: the level-2 kernel behind k_l6_matches"""
    cases = jc.group("len", 3) + jc.group("mod", 3) + jc.group("part", 3) + short_rounds(3)
    for fmt in (0, 1):
        for c in cases[fmt::2]:
            d = jc.data(c)
            _, got = encode(torch, xctx, dev(torch, d), c.n, fmt, lvl, c.P)
            check_stream(got, want(oracle, c, fmt, lvl), d, fmt, (jc.case_id(c), fmt, lvl))


@pytest.mark.parametrize("lvl", [1, 2])
def test_one_parser_kernels(torch, ctx, oracle, lvl):
    """k_encode_l1 / k_encode_l2_t<0, false> (what runs where the LDS-order probe's verdict is "does not hold", forced here as
    in test_gpu_planted.py): wave_adler on the emitter's wavefront"""
    try:
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_order(0)
        run_cases(torch, ctx, oracle, jc.group("len", lvl) + jc.group("mod", lvl) + jc.group("part", lvl) + short_rounds(lvl, 8193), 0, lvl)
    finally:
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


STREAM_LENGTHS = [1, 17, 65534, 65535, 65536, 2 * 65535 + 1, 3 * 65535 + 777, 3 * 32768 + 5, 2 * jc.ADLER_MOD]


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_encode_stream(torch, ctx, oracle, lvl, fmt):
    """the sequential stream: level 0's blocks of 65,535 bytes -- an odd size: coop_copy_adler's head and tail, the slicing path of
    the CRC -- and 32 KiB checksum chunks under k_adler_packets / k_crc32_packets at levels 1..3"""
    for fam in ("ff", "ffnoise", "impulse"):
        for n in STREAM_LENGTHS:
            c = jc.Case("stream", fam, n, 32768, n - 1 - n // 3 if fam == "impulse" else 6, ())
            d = jc.data(c)
            cap = 2 * n + 1024
            expect = oracle.encode(d, fmt, lvl, cap)
            assert jc.inflates(expect, d, fmt)
            dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            w = ctx.encode_stream(dev(torch, d), n, dst, cap, fmt, lvl)
            assert bool((dst[cap:] == 0xA5).all())
            check_stream(dst[:w].cpu().numpy().tobytes(), expect, d, fmt, (fam, n, fmt, lvl))


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
@pytest.mark.parametrize("lvl", [0, 2, 3])
def test_encode_ranges(torch, ctx, oracle, lvl, fmt):
    """the reference's own split: k_ranges_l0 / k_stream_l2 per range, the checksum over 32 KiB chunks beside them"""
    for fam in ("ff", "ffnoise", "impulse"):
        for n, count in ((2 * jc.ADLER_MOD + 1, 3), (200001, 7), (32768 * 5, 5), (65521, 61)):
            c = jc.Case("ranges", fam, n, 32768, n - 1 - n // 3 if fam == "impulse" else 8, ())
            d = jc.data(c)
            expect = oracle.encode_ranges(d, fmt, lvl, count)
            cap = 2 * n + 4096 + 16 * count
            dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            w = ctx.encode_ranges(dev(torch, d), n, dst, cap, count, fmt, lvl)
            assert bool((dst[cap:] == 0xA5).all())
            check_stream(dst[:w].cpu().numpy().tobytes(), expect, d, fmt, (fam, n, count, fmt, lvl))


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
def test_ranges_past_the_checksum_grids(torch, ctx, fmt):
    """the sequential and ranges forms sum fixed chunks of 32 KiB, so only a large input passes their grids: 4097 chunks and 5
    bytes of 0xFF at level 0 -- k_adler_packets' grid of 4096 and k_crc32_packets' of 2048, five chunks a thread in k_cks_reduce.
    (128 MiB: the stream is checked by zlib alone.)"""
    n = 4097 * 32768 + 5
    src = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    cap = n + (n // 65535 + 16) * 5 + 64
    dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    w = ctx.encode_ranges(src, n, dst, cap, 5, fmt, 0)
    assert bool((dst[cap:] == 0xA5).all())
    got = dst[:w].cpu().numpy().tobytes()
    d = b"\xFF" * n
    t = jc.trailer(d, fmt)
    assert got[-len(t):] == t, (got[-len(t):].hex(), t.hex())
    assert jc.inflates(got, d, fmt)


def batch_layout(torch, items, fmt, lvl):
    """sources back to back; destination i starts at 16-byte phase i of its own region, every region 0xA5 around it"""
    srcs, at = [], 0
    datas = [jc.data(c) for c in items]
    src = dev(torch, b"".join(datas))
    for d in datas:
        srcs.append((src.data_ptr() + at, len(d)))
        at += len(d)
    caps = [zz.bound(c.n, fmt, lvl, c.P) for c in items]
    region = (max(caps) + 16 + GUARD + 15) // 16 * 16
    dst = torch.full((len(items) * region,), 0xA5, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    offs = [i * region + GUARD // 2 + i % 16 for i in range(len(items))]
    return src, srcs, datas, dst, offs, caps, region


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["zlib", "gzip", "raw"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_encode_batch(torch, ctx, oracle, lvl, fmt):
    """k_batch_finalize strides an item's packets over a wavefront's lanes, batch_crc_fold takes runs of ceil(npk / 64): items of
    1, 63, 64, 65 and 130 packets, `ff`, `impulse` and `random` in one batch, destinations at every 16-byte phase"""
    items = jc.batch_items()
    src, srcs, datas, dst, offs, caps, region = batch_layout(torch, items, fmt, lvl)
    assert {(dst.data_ptr() + o) % 16 for o in offs} == set(range(16))
    lens = ctx.encode_batch(srcs, [(dst.data_ptr() + o, cap) for o, cap in zip(offs, caps)], fmt, lvl, jc.BATCH_P)
    assert None not in lens
    host = dst.cpu().numpy().tobytes()
    for i, c in enumerate(items):
        got = host[offs[i]: offs[i] + lens[i]]
        check_stream(got, want(oracle, c, fmt, lvl), datas[i], fmt, (jc.case_id(c), fmt, lvl))
        assert host[i * region: offs[i]] == b"\xA5" * (offs[i] - i * region)
        assert host[offs[i] + lens[i]: (i + 1) * region] == b"\xA5" * ((i + 1) * region - offs[i] - lens[i])


MEMBERS_B, MEMBERS_P = 40000, 512


def members_data():
    return b"\xFF" * MEMBERS_B + jc.data(jc.Case("m", "random", MEMBERS_B, MEMBERS_P, 11, ())) + \
        jc.data(jc.Case("m", "impulse", MEMBERS_B, MEMBERS_P, MEMBERS_B - 700, ())) + b"\xFF" * 1234


def members_file(torch, ctx, d, lvl):
    cap = zz.members_bound(len(d), MEMBERS_B, MEMBERS_P, True)
    dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    w = ctx.encode_members(dev(torch, d), len(d), dst, cap, lvl, MEMBERS_B, MEMBERS_P, True)
    assert bool((dst[cap:] == 0xA5).all())
    return dst[:w].cpu().numpy().tobytes()


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_encode_members(torch, ctx, oracle, lvl):
    """k_mw_finalize folds a member's CRC-32 with batch_crc_fold: P = 512 gives a member of 40,000 bytes 79 packets, runs of two"""
    assert -(-MEMBERS_B // MEMBERS_P) > 64
    d = members_data()
    got = members_file(torch, ctx, d, lvl)
    expect, offsets, _ = mw.expected(oracle, d, lvl, MEMBERS_B, MEMBERS_P, True)
    assert got == expect
    # every member's CRC-32 and ISIZE by zlib alone
    for k, (at, size) in enumerate(mw.members_of(got)[:-1]):
        block = d[k * MEMBERS_B: (k + 1) * MEMBERS_B]
        assert got[at + size - 8: at + size] == jc.trailer(block, 1), k


MULTI = [("ffnoise", 1024, 37 * 1024 + 5, (1, 30)), ("ff", 16, 2048 * 16 + 7, (1025, 1030)), ("ffnoise", 24, 2049 * 24, (3, 1100))]


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_encode_multi_uneven_shards(torch, oracle, lvl, fmt):
    """zz_encode_multi_device on one device: three shards of uneven length, their partials folded on the host with
    adler_combine / crc32_combine"""
    ctxs = [zz.Context(0) for _ in range(3)]
    try:
        for fam, P, n, cut in MULTI:
            c = jc.Case("multi", fam, n, P, 12, ())
            d = jc.data(c)
            cuts = [0, cut[0] * P, cut[1] * P, n]
            keep, srcs, ns, halos = [], [], [], []
            for lo, hi in zip(cuts, cuts[1:]):
                h = min(65536, lo)
                t = dev(torch, d[lo - h:hi])
                keep.append(t)
                srcs.append(t[h:])
                ns.append(hi - lo)
                halos.append(h)
            cap = zz.bound(n, fmt, lvl, P)
            dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            w = zz.encode_multi(ctxs, srcs, ns, dst, cap, fmt, lvl, P, halos=halos)
            assert bool((dst[cap:] == 0xA5).all())
            check_stream(dst[:w].cpu().numpy().tobytes(), oracle.encode_packets(d, fmt, lvl, P), d, fmt, (fam, P, n, fmt, lvl))
    finally:
        for c in ctxs:
            c.close()


# ---- shard partials ---------------------------------------------------------------------------------------------------

SHARDS = [("ffnoise", 1024, 40 * 1024 + 77), ("ff", 32768, 5 * 32768 + 9), ("ffnoise", 16, 2048 * 16 + 3), ("ff", 24, 2049 * 24),
          ("impulse", 33, 1100 * 33 + 1)]


def shard_cuts(k, parts):
    """packet counts at which k >= 6 packets are cut into `parts` uneven shards"""
    return [0, k // 2 + 1, k] if parts == 2 else sorted({0, 1, k // 5 + 1, k // 2 + 1, k - 1, k})


def shard_expected(oracle, raw, view, h, ln, P, lvl, last):
    """the oracle's packets of view[h, h + ln): what lies in front of them, the halo, is all the shard's encoder may look back at"""
    out = []
    for off in range(0, ln, P):
        l = min(P, ln - off)
        w = oracle.L.zzo_packet_warm(lvl, view, h + off, l, int(last and off + l == ln), raw, len(raw), 0)
        out.append(ctypes.string_at(raw, w))
    return b"".join(out)


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3, 4, 5, 6])
def test_shard_partials(torch, xctx, oracle, lvl, fmt):
    """encode_shard's partial is zlib's value for the shard's bytes -- Adler-32 with start value 0, the plain CRC-32 --, and the
    fold of the partials is the whole trailer. The source buffer starts at an odd address and every shard is given 1, 3 or 15
    bytes of halo in front (in front of the first one they are not the stream's): a shard's bytes are the oracle's packets over
    the same view -- backward extension and the windows of levels 4..6 end where the halo does --, and the shards one after the
    other inflate to the input."""
    raw = ctypes.create_string_buffer(2 * 32768 + 1024)
    for fam, P, n in SHARDS:
        c = jc.Case("shard", fam, n, P, n - 40 if fam == "impulse" else 13, ())
        d = jc.data(c)
        k = jc.npk(c)
        for parts in (2, 5):
            for odd in (1, 3, 15):
                whole = b"\xEE" * odd + d
                buf = dev(torch, whole)
                assert (buf.data_ptr() + odd) % 2 == 1
                cuts = [min(x * P, n) for x in shard_cuts(k, parts)]
                assert len(cuts) == parts + 1 and cuts == sorted(set(cuts)) and cuts[-1] == n
                cap = zz.bound(n, 2, min(lvl, 3), P)
                dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                at, adler, crc, ends = 0, 1, 0, [0]
                for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
                    halo = min(lo + odd, (1, 3, 15)[(i + odd) % 3])
                    w, cks = xctx.encode_shard(buf.data_ptr() + odd + lo, hi - lo, dst.data_ptr() + at, cap - at, halo=halo,
                                               is_last=hi == n, checksum=fmt, level=lvl, packet_size=P)
                    piece = d[lo:hi]
                    what = (fam, P, n, parts, odd, i, lvl, fmt)
                    assert cks == jc.partial(piece, fmt), what
                    if fmt == 0:
                        assert zz.combine(1, cks, hi - lo) == zlib.adler32(piece), what
                        adler = zz.combine(adler, cks, hi - lo)
                    else:
                        crc = zz.crc32_combine(crc, cks, hi - lo)
                    at += w
                    ends.append(at)
                assert (adler if fmt == 0 else crc) == (zlib.adler32(d) if fmt == 0 else zlib.crc32(d)), (fam, P, parts, odd)
                assert bool((dst[cap:] == 0xA5).all())
                got = dst[:at].cpu().numpy().tobytes()
                for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
                    halo = min(lo + odd, (1, 3, 15)[(i + odd) % 3])
                    view = whole[odd + lo - halo: odd + hi]
                    assert got[ends[i]:ends[i + 1]] == shard_expected(oracle, raw, view, halo, hi - lo, P, lvl, hi == n), \
                        (fam, P, parts, odd, i, lvl)
                assert jc.inflates(got, d, 2), (fam, P, parts, odd, lvl)


# ---- decode -----------------------------------------------------------------------------------------------------------

def decode_case(torch, ctx, oracle, c, fmt, lvl):
    """encode on the device (the index comes from the call), then every path of Context.decode; (stream bytes, input) back"""
    d = jc.data(c)
    src = dev(torch, d)
    stream, got = encode(torch, ctx, src, c.n, fmt, lvl, c.P)
    idx = ctx.packet_index()
    paths = [(c.P, idx)] + ([(c.P, None), (0, None)] if c.n <= SMALL else [])
    for P, index in paths:
        out = torch.full((c.n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        w = ctx.decode(stream, len(got), out, c.n, fmt, P, index)
        assert w == c.n and torch.equal(out[:c.n], src[:c.n]) and bool((out[c.n:] == 0xA5).all()), (jc.case_id(c), fmt, lvl, P)
        if index is not None:
            assert ctx.last_decode_path() == zz.DECODE_INDEXED
    return got, d


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
@pytest.mark.parametrize("lvl", [0, 1, 2])
def test_decode_paths_and_batch(torch, ctx, oracle, lvl, fmt):
    """the list's streams back through Context.decode -- indexed, discovered and serial -- and, as the items of one call, through
    decode_batch (zi_adler_lanes / zi_crc_lanes); gzip streams also through decode_members"""
    cases = jc.group("len", lvl)[::3] + jc.group("mod", lvl) + jc.group("part", lvl)[::5] + jc.group("crc", lvl)[::2] + \
        [c for c in jc.group("round", lvl) if c.family != "ff" or jc.npk(c) > 60000]
    streams = []
    for c in cases:
        got, d = decode_case(torch, ctx, oracle, c, fmt, lvl)
        if c.n <= SMALL:
            streams.append((got, d))
    src = dev(torch, b"".join(s for s, _ in streams))
    total = sum(len(d) + GUARD for _, d in streams)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    srcs, dsts, at, to = [], [], 0, 0
    for s, d in streams:
        srcs.append((src.data_ptr() + at, len(s)))
        dsts.append((out.data_ptr() + to, len(d)))
        at += len(s)
        to += len(d) + GUARD
    lens, status = ctx.decode_batch(srcs, dsts, fmt)
    assert status == [0] * len(streams) and lens == [len(d) for _, d in streams]
    assert out.cpu().numpy().tobytes() == b"".join(d + b"\xA5" * GUARD for _, d in streams)
    if fmt == 1:
        for s, d in streams[::4]:
            o = torch.full((len(d) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            assert ctx.decode_members(dev(torch, s), len(s), o, len(d)) == len(d)
            assert o.cpu().numpy().tobytes() == d + b"\xA5" * GUARD


@pytest.mark.parametrize("lvl", [0, 2])
def test_decode_members_of_blocked_files(torch, ctx, lvl):
    d = members_data()
    f = members_file(torch, ctx, d, lvl)
    o = torch.full((len(d) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ctx.decode_members(dev(torch, f), len(f), o, len(d)) == len(d)
    assert o.cpu().numpy().tobytes() == d + b"\xA5" * GUARD
    assert ctx.last_decode_members_stats()[2] == zz.MEMBERS_BLOCKED


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
def test_decode_trailer_fold_past_1024_chunks(torch, ctx, fmt):
    """dec_check_trailer sums the decoded bytes in 32 KiB chunks and folds them with k_cks_reduce: 1025 chunks and 77 bytes of 0xFF
    give its threads a run of two. Encoded on the device at P = 32768, decoded with the call's index, compared on the device."""
    n = 1025 * 32768 + 77
    src = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    stream, got = encode(torch, ctx, src, n, fmt, 1, 32768)
    d = b"\xFF" * n
    t = jc.trailer(d, fmt)
    assert got[-len(t):] == t
    idx = ctx.packet_index()
    out = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ctx.decode(stream, len(got), out, n, fmt, 32768, idx) == n
    assert torch.equal(out[:n], src) and bool((out[n:] == 0xA5).all())
    # and its trailer off by one is found there
    for what, bad in jc.bad_trailers(got[-16:], fmt):
        b = stream.clone()
        b[-16:] = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
        with pytest.raises(zz.ZzFlateError) as e:
            ctx.decode(b, len(got), out, n, fmt, 32768, idx)
        assert e.value.code == zz.E_DATA, what
        assert bool((out[n:] == 0xA5).all())


def test_decode_batch_item_of_four_mib(torch, ctx):
    """one wavefront sums 4 MiB + 65,524 bytes of 0xFF: every lane of zi_adler_lanes takes its outer loop a second time"""
    n = jc.ITEM_LENGTH_64_LANES
    for fmt in (0, 1):
        d, s = jc.item_stream("ff", n, fmt)
        streams = [s] + [b for _, b in jc.bad_trailers(s, fmt)]
        src = [dev(torch, b) for b in streams]
        out = torch.full((len(streams) * (n + GUARD),), 0xA5, dtype=torch.uint8, device="cuda")
        lens, status = ctx.decode_batch([(t.data_ptr(), len(b)) for t, b in zip(src, streams)],
                                        [(out.data_ptr() + i * (n + GUARD), n) for i in range(len(streams))], fmt)
        assert status == [0, zz.E_DATA, zz.E_DATA] and lens[0] == n, (fmt, status, lens)
        view = out.view(len(streams), n + GUARD)
        assert bool((view[0, :n] == 0xFF).all()) and bool((view[:, n:] == 0xA5).all())


BAD = [("ffnoise", 32768, 2 * jc.ADLER_MOD + 1, 1), ("ff", 16, 1025 * 16, 1), ("ffnoise", 4096, 3 * 4096 + 5, 2), ("impulse", 1000, 70001, 0)]


@pytest.mark.parametrize("fmt", [0, 1], ids=["zlib", "gzip"])
def test_a_trailer_off_by_one_is_data_error_on_every_path(torch, ctx, fmt):
    """the Adler-32's low half, its high half, the CRC-32 or ISIZE off by one: E_DATA from the indexed, the discovered and the
    serial path of decode, from decode_batch and from decode_members, and nothing written outside the destination"""
    for fam, P, n, lvl in BAD:
        c = jc.Case("bad", fam, n, P, n // 2 if fam == "impulse" else 14, ())
        d = jc.data(c)
        stream, got = encode(torch, ctx, dev(torch, d), n, fmt, lvl, P)
        idx = ctx.packet_index()
        bad = jc.bad_trailers(got, fmt)
        assert len(bad) == 2
        for what, b in bad:
            assert not jc.inflates(b, d, fmt)
            t = dev(torch, b)
            for P2, index in ((P, idx), (P, None), (0, None)):
                out = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                with pytest.raises(zz.ZzFlateError) as e:
                    ctx.decode(t, len(b), out, n, fmt, P2, index)
                assert e.value.code == zz.E_DATA, (fam, P, what, P2)
                assert bool((out[n:] == 0xA5).all())
            out = torch.full((2 * (n + GUARD),), 0xA5, dtype=torch.uint8, device="cuda")
            lens, status = ctx.decode_batch([(t.data_ptr(), len(b)), (stream.data_ptr(), len(got))],
                                            [(out.data_ptr(), n), (out.data_ptr() + n + GUARD, n)], fmt)
            assert status == [zz.E_DATA, 0] and lens[1] == n, (fam, P, what, status)
            host = out.cpu().numpy().tobytes()
            assert host[n:n + GUARD] == b"\xA5" * GUARD and host[n + GUARD:] == d + b"\xA5" * GUARD
            if fmt == 1:
                out = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                with pytest.raises(zz.ZzFlateError) as e:
                    ctx.decode_members(t, len(b), out, n)
                assert e.value.code == zz.E_DATA, (fam, P, what)
                assert bool((out[n:] == 0xA5).all())
