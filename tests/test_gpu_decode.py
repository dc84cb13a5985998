"""Decode on the device (zz_decode_device): round trips through the indexed, discovered and serial paths, streams made
by the oracle, by Python's zlib / gzip and by the library's other encoders, errors, and full-size calls."""
import gzip
import os
import random
import zlib

import pytest

from conftest import CORPUS, SYNTH_KINDS, Oracle, synth

torch = pytest.importorskip("torch")
import zzflate_amd as zz  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = zz.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def xctx():
    c = zz.Context(0)
    c.set_extended_levels(True)
    yield c
    c.close()


def dev(data):
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def encode(c, src, n, fmt, lvl, P):
    cap = zz.bound(n, fmt, min(lvl, 3), P) + 64
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = c.encode(src, n, dst, cap, fmt, lvl, P)
    return dst[:w].clone(), w


def decode(c, stream, w, n, fmt, P, index=None, slack=64):
    cap = n + slack
    out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    got = c.decode(stream, w, out, cap, fmt, P, index)
    return out, got


def roundtrip(c, data, fmt, lvl, P, path=zz.DECODE_INDEXED):
    n = len(data)
    src = dev(data)
    stream, w = encode(c, src, n, fmt, lvl, P)
    idx = c.packet_index()
    out, got = decode(c, stream, w, n, fmt, P, idx)
    assert got == n
    assert torch.equal(out[:n], src[:n])
    assert c.last_decode_path() == path
    return stream, w, idx


def corpus_file(name):
    return open(os.path.join(CORPUS, name), "rb").read()


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_roundtrip_corpus(ctx, lvl, fmt):
    for name in ("alice29.txt", "kennedy.xls", "ptt5", "fields.c"):
        roundtrip(ctx, corpus_file(name), fmt, lvl, 32768)


@pytest.mark.parametrize("kind", SYNTH_KINDS + ["longperiod"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_roundtrip_synthetic(ctx, kind, lvl):
    for P in (32768, 4096):
        roundtrip(ctx, synth(kind, 100000, 3), 0, lvl, P)


@pytest.mark.parametrize("P", [32768, 4096, 1000, 1])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_roundtrip_sizes(ctx, P, lvl):
    base = synth("words", 3 * max(P, 1000) + 10, 5)
    for n in sorted({0, 1, max(P - 1, 0), P, P + 1}):
        roundtrip(ctx, base[:n], 0 if n % 2 else 1, lvl, P)


@pytest.mark.parametrize("warm", [4096, 32768])
@pytest.mark.parametrize("lvl", [1, 2, 3])
def test_roundtrip_warm(lvl, warm):
    c = zz.Context(0)
    c.set_warm_window(warm)
    data = corpus_file("lcet10.txt") + synth("period", 50000, 7)
    for P in (32768, 4096, 1000):
        roundtrip(c, data, 1, lvl, P)
    c.close()


@pytest.mark.parametrize("lvl", [4, 5, 6])
def test_roundtrip_extended(xctx, lvl):
    data = corpus_file("alice29.txt") + synth("period", 60000, 2) + corpus_file("kennedy.xls")[:100000]
    for P in (32768, 4096, 1000):
        for fmt in (0, 1, 2):
            roundtrip(xctx, data, fmt, lvl, P)


def test_pending_bytes_are_resolved(xctx):
    """Periodic data at level 6 with small packets: almost every packet copies from the one in front of it."""
    data = synth("period", 300000, 11)
    roundtrip(xctx, data, 0, 6, 1000)
    pend, rounds = xctx.last_decode_stats()
    assert pend > 100000 and rounds >= 2


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_discovery_recovers_the_index(ctx, lvl):
    for P in (32768, 4096, 1000):
        data = corpus_file("lcet10.txt")[: 5 * P + 17] if P > 1000 else synth("words", 20000, 1)
        stream, w, idx = roundtrip(ctx, data, 0, lvl, P)
        out, got = decode(ctx, stream, w, len(data), 0, P, None)
        assert got == len(data) and torch.equal(out[: len(data)], dev(data)[: len(data)])
        assert ctx.last_decode_path() == zz.DECODE_DISCOVERED
        assert torch.equal(ctx.last_decode_index(), idx)


def marker_data(n, seed):
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.getrandbits(8) for _ in range(rng.randint(500, 3000))) + b"\x01\x00\xfe\xff" + bytes([rng.getrandbits(8)])
    return bytes(out[:n])


@pytest.mark.parametrize("lvl", [0, 2])
def test_discovery_with_markers_inside_stored_data(ctx, lvl):
    """False candidates (the marker inside stored bytes) are walked over and phase 1 runs again on the recovered index,
    with a destination just the size of the output."""
    data = marker_data(150000, lvl)
    src = dev(data)
    for P in (32768, 4096):
        stream, w = encode(ctx, src, len(data), 0, lvl, P)
        idx = ctx.packet_index()
        assert bytes(stream.cpu().numpy()).count(b"\x01\x00\xfe\xff") > len(data) // P + 10
        for slack in (0, 64):
            out, got = decode(ctx, stream, w, len(data), 0, P, None, slack=slack)
            assert got == len(data) and torch.equal(out[: len(data)], src)
            assert ctx.last_decode_path() == zz.DECODE_DISCOVERED
            assert torch.equal(ctx.last_decode_index(), idx)


def test_nospace_is_found_by_the_parallel_paths(ctx):
    data = corpus_file("lcet10.txt")
    src = dev(data)
    n = len(data)
    stream, w = encode(ctx, src, n, 0, 2, 4096)
    idx = ctx.packet_index()
    for cap in (n - 1, n - 5000, 100):
        for index in (idx, None):
            out = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            expect(zz.E_NOSPACE, lambda: ctx.decode(stream, w, out, cap, 0, 4096, index))
            assert bool((out[cap:] == 0x5A).all())
            assert "destination too small for the decoded stream (%d bytes)" % n in zz.lib.zz_last_error().decode()


def test_index_must_be_an_int64_tensor_on_the_device(ctx):
    data = corpus_file("fields.c")
    src = dev(data)
    stream, w = encode(ctx, src, len(data), 0, 1, 4096)
    idx = ctx.packet_index()
    out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        ctx.decode(stream, w, out, len(data) + 64, 0, 4096, idx.to(torch.int32))
    with pytest.raises(TypeError):
        ctx.decode(stream, w, out, len(data) + 64, 0, 4096, torch.stack([idx, idx], 1)[:, 0])
    with pytest.raises(ValueError):
        ctx.decode(stream, w, out, len(data) + 64, 0, 4096, idx.cpu())
    assert ctx.decode(stream, w, out, len(data) + 64, 0, 4096, idx) == len(data)


def test_candidates_over_the_cap_go_serial(ctx):
    data = b"\x01\x00\xfe\xff" * 20000
    src = dev(data)
    stream, w = encode(ctx, src, len(data), 0, 0, 32768)
    out, got = decode(ctx, stream, w, len(data), 0, 32768, None)
    assert got == len(data) and torch.equal(out[: len(data)], src)
    assert ctx.last_decode_path() == zz.DECODE_SERIAL


def oracle_index(o, data, lvl, P):
    import numpy as np
    offs, at = [0], 0
    npk = max(1, (len(data) + P - 1) // P)
    for k in range(npk):
        ln = min(P, len(data) - k * P)
        at += len(o.packet(data, lvl, k * P, ln, k == npk - 1))
        offs.append(at)
    return torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_oracle_streams_all_paths(ctx, lvl):
    o = Oracle()
    for name, P in (("alice29.txt", 32768), ("kennedy.xls", 4096), ("fields.c", 1000)):
        data = corpus_file(name)
        s = o.encode_packets(data, 0, lvl, P)
        idx = oracle_index(o, data, lvl, P)
        assert int(idx[-1]) == len(s) - 6
        st = dev(s)
        for P2, index, path in ((P, idx, zz.DECODE_INDEXED), (P, None, zz.DECODE_DISCOVERED), (0, None, zz.DECODE_SERIAL)):
            out, got = decode(ctx, st, len(s), len(data), 0, P2, index)
            assert got == len(data) and bytes(out[: len(data)].cpu().numpy()) == data
            assert ctx.last_decode_path() == path


@pytest.mark.parametrize("lvl", [0, 1, 6, 9])
def test_serial_python_zlib_and_gzip(ctx, lvl):
    data = corpus_file("alice29.txt") + corpus_file("ptt5")
    for wbits, fmt in ((15, 0), (31, 1), (-15, 2)):
        co = zlib.compressobj(lvl, zlib.DEFLATED, wbits)
        s = co.compress(data) + co.flush()
        for P in (0, 32768):
            out, got = decode(ctx, dev(s), len(s), len(data), fmt, P)
            assert got == len(data) and bytes(out[: len(data)].cpu().numpy()) == data
            # (with a packet size, discovery may take a stream whose blocks happen to line up with it)
            assert ctx.last_decode_path() == zz.DECODE_SERIAL or P
    s = gzip.compress(data, compresslevel=max(lvl, 1))
    out, got = decode(ctx, dev(s), len(s), len(data), 1, 0)
    assert bytes(out[: len(data)].cpu().numpy()) == data


def test_gzip_header_fields(ctx):
    data = corpus_file("fields.c")
    body = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = body.compress(data) + body.flush()
    hdr = bytearray(b"\x1f\x8b\x08\x1e\x00\x00\x00\x00\x00\xff")   # FEXTRA FNAME FCOMMENT FHCRC
    hdr += b"\x03\x00abc" + b"name.txt\x00" + b"a comment\x00"
    crc = zlib.crc32(bytes(hdr)) & 0xFFFF
    hdr += bytes([crc & 0xFF, crc >> 8])
    s = bytes(hdr) + raw + zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little")
    out, got = decode(ctx, dev(s), len(s), len(data), 1, 0)
    assert got == len(data) and bytes(out[:got].cpu().numpy()) == data


@pytest.mark.parametrize("lvl", [0, 2, 3])
def test_serial_sequential_and_ranges_streams(ctx, lvl):
    data = corpus_file("lcet10.txt")
    src = dev(data)
    cap = 2 * len(data) + 4096
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode_stream(src, len(data), dst, cap, 0, lvl)
    for P in (0, 32768):
        out, got = decode(ctx, dst[:w].clone(), w, len(data), 0, P)
        assert got == len(data) and torch.equal(out[: len(data)], src)
    w = ctx.encode_ranges(src, len(data), dst, cap, 7, 1, lvl)
    out, got = decode(ctx, dst[:w].clone(), w, len(data), 1, 0)
    assert got == len(data) and torch.equal(out[: len(data)], src)
    assert ctx.last_decode_path() == zz.DECODE_SERIAL


def expect(code, fn):
    with pytest.raises(zz.ZzFlateError) as e:
        fn()
    assert e.value.code == code, str(e.value)


def test_errors(ctx):
    data = corpus_file("alice29.txt")
    src = dev(data)
    n = len(data)
    for fmt in (0, 1):
        stream, w = encode(ctx, src, n, fmt, 2, 4096)
        idx = ctx.packet_index()
        raw = bytearray(stream.cpu().numpy().tobytes())
        bad = bytearray(raw); bad[-(4 if fmt == 0 else 8)] ^= 0x40            # the checksum
        expect(zz.E_DATA, lambda: decode(ctx, dev(bytes(bad)), w, n, fmt, 4096, idx))
        expect(zz.E_DATA, lambda: decode(ctx, stream, w - 3, n, fmt, 4096, idx))        # truncated
        expect(zz.E_DATA, lambda: decode(ctx, dev(bytes(raw) + b"\x00"), w + 1, n, fmt, 4096, idx))   # trailing byte
        # too small a destination: an error, and nothing written past cap
        small = n // 2
        out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        expect(zz.E_NOSPACE, lambda: ctx.decode(stream, w, out, small, fmt, 4096, idx))
        assert bool((out[small:] == 0xA5).all())
        out.fill_(0xA5)
        expect(zz.E_NOSPACE, lambda: ctx.decode(stream, w, out, small, fmt, 0, None))
        assert bool((out[small:] == 0xA5).all())
    stream, w = encode(ctx, src, n, 1, 1, 32768)
    raw = bytearray(stream.cpu().numpy().tobytes())
    raw[-4] ^= 1                                                              # ISIZE
    expect(zz.E_DATA, lambda: decode(ctx, dev(bytes(raw)), w, n, 1, 32768, ctx.packet_index()))
    fdict = b"\x78\xbb" + b"\x00" * 8
    assert (0x78 * 256 + 0xBB) % 31 == 0
    expect(zz.E_UNSUPPORTED, lambda: decode(ctx, dev(fdict), len(fdict), 10, 0, 0))


def test_non_first_shard_is_too_far_back(ctx):
    data = synth("period", 200000, 4)
    src = dev(data)
    P = 32768
    half = 3 * P
    cap = zz.bound(len(data), 2, 2, P)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w, _ = ctx.encode_shard(src[half:], len(data) - half, dst, cap, halo=half, is_last=True, checksum=zz.Format.Deflate,
                            level=2, packet_size=P)
    expect(zz.E_DATA, lambda: decode(ctx, dst[:w].clone(), w, len(data), 2, 0))


def test_garbage_gives_errors(ctx):
    rng = random.Random(5)
    base = zlib.compress(corpus_file("grammar.lsp"), 6)
    cases = [bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 3000))) for _ in range(12)]
    cases += [base[:k] for k in range(0, len(base), max(1, len(base) // 40))]
    for i in range(0, len(base), 7):
        b = bytearray(base); b[i] ^= 1 << (i % 8); cases.append(bytes(b))
    for s in cases:
        for fmt in (0, 1, 2):
            for P in (0, 32768, 1000):
                try:
                    decode(ctx, dev(s), len(s), 8192, fmt, P, slack=0)
                except zz.ZzFlateError as e:
                    assert e.code in (zz.E_DATA, zz.E_NOSPACE, zz.E_UNSUPPORTED)


EDGE_P = 64
EDGE_PACKETS = (1 << 18) + 3       # at P <= 256 a batch holds 2^18 packets: the smallest stream that takes two batches


def test_indexed_decode_across_the_batch_edge(ctx):
    """Every packet copies from the one in front of it, the second batch's first packets from the first batch's last."""
    from deflate_cases import foreign_packets
    rng = random.Random(41)
    period = bytes(rng.getrandbits(8) for _ in range(97))
    n = EDGE_PACKETS * EDGE_P - 5
    data = (period * (n // 97 + 1))[:n]
    s, index, _ = foreign_packets(data, EDGE_P, 9, zlib.Z_DEFAULT_STRATEGY, window=512)
    assert len(index) == EDGE_PACKETS + 1
    stream, idx = dev(s), torch.tensor(index, dtype=torch.int64).cuda()
    out, got = decode(ctx, stream, len(s), n, 0, EDGE_P, idx)
    assert got == n and torch.equal(out[:n], dev(data))
    assert ctx.last_decode_path() == zz.DECODE_INDEXED
    assert ctx.last_decode_stats()[0] > 0
    out.fill_(0x5A)
    expect(zz.E_NOSPACE, lambda: ctx.decode(stream, len(s), out, n - 1, 0, EDGE_P, idx))
    assert bool((out[n - 1:] == 0x5A).all())


def test_discovery_with_more_candidates_than_a_batch(ctx):
    n = EDGE_PACKETS * EDGE_P - 5
    data = synth("words", n, 17)
    src = dev(data)
    stream, w = encode(ctx, src, n, 0, 1, EDGE_P)
    idx = ctx.packet_index()
    assert idx.numel() == EDGE_PACKETS + 1
    out, got = decode(ctx, stream, w, n, 0, EDGE_P, None)
    assert got == n and torch.equal(out[:n], src)
    assert ctx.last_decode_path() == zz.DECODE_DISCOVERED
    assert torch.equal(ctx.last_decode_index(), idx)


def every_path_calls():
    """(name, call) for every decode entry point, on inputs made once: call(context) -> a value that compares (bytes, lengths,
    statuses). 300,000 bytes in packets of 1000."""
    P, n = 1000, 300000
    data = synth("words", 200000, 23) + synth("period", n - 200000, 23)
    src = dev(data)
    b = zz.Context(0)
    stream, w = encode(b, src, n, 0, 2, P)
    idx = b.packet_index()
    cks = b.packet_checksums(src, n, 0, P)
    foreign = zlib.compress(data, 6)
    fsrc = dev(foreign)
    points, pn = zz.points_index_host(foreign, zz.Format.Zlib, 16384)
    assert pn == n
    items = [zlib.compress(data[3000 * i: 3000 * (i + 1) + i], 6) for i in range(40)]
    isrcs = [dev(s) for s in items]
    icaps = [3000 + i if i != 7 else 100 for i in range(40)]
    mcap = zz.members_bound(n)
    mfile = torch.zeros(mcap, dtype=torch.uint8, device="cuda")
    mw = b.encode_members(src, n, mfile, mcap, level=1)
    midx = b.members_index(mfile, mw)
    b.close()
    firsts, lens = [0, 999, 150000, n - 500, n + P], [10, 2002, 40000, 1000, 5]

    def whole(P2, index):
        def call(c):
            out, got = decode(c, stream, w, n, 0, P2, index)
            return got, bytes(out[:got].cpu().numpy()), c.last_decode_path(), c.last_decode_stats()
        return call

    def by_points(c):
        out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        got = c.decode_points(fsrc, len(foreign), out, n, points, zz.Format.Zlib)
        return got, bytes(out[:got].cpu().numpy()), c.last_decode_path(), c.last_decode_stats()

    def one_range(checked):
        def call(c):
            out = torch.zeros(70000, dtype=torch.uint8, device="cuda")
            if checked:
                got = c.decode_range_checked(stream, w, out, 70000, 123456, 70000, cks, n, 0, P, idx)
            else:
                got = c.decode_range(stream, w, out, 70000, 123456, 70000, 0, P, idx)
            return got, bytes(out[:got].cpu().numpy()), c.last_decode_range_stats()
        return call

    def many_ranges(checked):
        def call(c):
            outs = [torch.zeros(ln, dtype=torch.uint8, device="cuda") for ln in lens]
            if checked:
                got, status = c.decode_ranges_checked(stream, w, firsts, lens, outs, cks, n, None, 0, P, idx)
            else:
                got, status = c.decode_ranges(stream, w, firsts, lens, outs, None, 0, P, idx)
            return got, status, [bytes(o.cpu().numpy()) for o in outs], c.last_decode_ranges_stats()
        return call

    def batch(c):
        outs = [torch.zeros(3100, dtype=torch.uint8, device="cuda") for _ in items]
        got, status = c.decode_batch(isrcs, outs, zz.Format.Zlib, icaps)
        return got, status, [bytes(o[:g].cpu().numpy()) for o, g in zip(outs, got) if g is not None]

    def members(c):
        out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        got = c.decode_members(mfile, mw, out, n)
        return got, bytes(out[:got].cpu().numpy()), c.last_decode_members_stats()

    def members_index(c):
        return c.members_index(mfile, mw).cpu().tolist()

    def members_ranges(c):
        outs = [torch.zeros(ln, dtype=torch.uint8, device="cuda") for ln in lens]
        got, status = c.decode_members_ranges(mfile, mw, midx, firsts, lens, outs)
        return got, status, [bytes(o.cpu().numpy()) for o in outs], c.last_decode_members_ranges_stats()

    return [("decode indexed", whole(P, idx)), ("decode discovered", whole(P, None)), ("decode serial", whole(0, None)),
            ("decode_points", by_points), ("decode_range", one_range(False)), ("decode_range_checked", one_range(True)),
            ("decode_ranges", many_ranges(False)), ("decode_ranges_checked", many_ranges(True)), ("decode_batch", batch),
            ("decode_members", members), ("members_index", members_index), ("decode_members_ranges", members_ranges)], data


@pytest.fixture(scope="module")
def every_path():
    """The calls, and what each gives on a context of its own."""
    calls, data = every_path_calls()
    fresh = {}
    for name, call in calls:
        c = zz.Context(0)
        fresh[name] = call(c)
        c.close()
    # the references are the data's own bytes, whichever path made them
    for name in ("decode indexed", "decode discovered", "decode serial", "decode_points", "decode_members"):
        assert fresh[name][:2] == (len(data), data), name
    assert [fresh[name][2] for name in ("decode indexed", "decode discovered", "decode serial", "decode_points")] == \
        [zz.DECODE_INDEXED, zz.DECODE_DISCOVERED, zz.DECODE_SERIAL, zz.DECODE_POINTS]
    assert fresh["decode_range"][:2] == (70000, data[123456:193456]) and fresh["decode_range_checked"][:2] == fresh["decode_range"][:2]
    for name in ("decode_ranges", "decode_ranges_checked", "decode_members_ranges"):
        got, status, outs = fresh[name][:3]
        assert got == [10, 2002, 40000, 500, None] and status == [0, 0, 0, 0, zz.E_ARG], name
        assert all(o[:g] == data[f:f + g] for o, g, f in zip(outs, got, (0, 999, 150000, len(data) - 500))), name
    assert fresh["decode_batch"][1] == [0 if i != 7 else zz.E_NOSPACE for i in range(40)]
    return calls, fresh


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_one_context_every_decode_path(every_path, order):
    """The paths share the context's buffers: a call after a smaller (or larger) one of another path gives what it gives alone."""
    calls, fresh = every_path
    c = zz.Context(0)
    for name, call in (calls if order == "listed" else calls[::-1]):
        assert call(c) == fresh[name], name
    c.close()


GIB = 1 << 30


@pytest.mark.parametrize("kind,n,lvl,fmt", [(zz.GEN_TEXT, GIB, 1, 0), (zz.GEN_TEXT, GIB, 2, 0), (zz.GEN_MIX, 2 * GIB, 3, 0),
                                            (zz.GEN_MIX, 2 * GIB, 6, 0), (zz.GEN_LOG, GIB, 2, 1)])
def test_full_size(xctx, kind, n, lvl, fmt):
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    xctx.generate(kind, 1, 0, src, n)
    stream, w = encode(xctx, src, n, fmt, lvl, 32768)
    idx = xctx.packet_index()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    got = xctx.decode(stream, w, out, n, fmt, 32768, idx)
    assert got == n and torch.equal(out, src)
    assert xctx.last_decode_path() == zz.DECODE_INDEXED
    del out, stream, src
    torch.cuda.empty_cache()
