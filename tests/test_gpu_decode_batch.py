"""zz_decode_batch_device / Context.decode_batch: many independent streams back to their bytes in one call, one wavefront per
stream. Every item decodes to the bytes that were compressed (never to what the code under test says they were), to what one
Context.decode call per item gives, and a damaged item gets its own status and leaves the others complete. Needs a real
MI355X: run with `-m gpu`."""
import ctypes
import gzip
import random
import zlib

import pytest

import zzflate_amd as zz
from conftest import CORPUS_FILES, SYNTH_KINDS, synth

pytestmark = pytest.mark.gpu
WBITS = {0: 15, 1: 31, 2: -15}
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def item_set(corpus, P, seed):
    """the item set of tests/test_gpu_batch.py: the corpus, every synth family, and the sizes around the packet edges, shuffled"""
    rng = random.Random(seed)
    items = [corpus[f] for f in CORPUS_FILES]
    sizes = [0, 1, 2, 63, 64, 65, P - 1, P, P + 1, 3 * P + 7, (1 << 20) + 13]
    for i, n in enumerate(sizes):
        items.append(synth(SYNTH_KINDS[i % len(SYNTH_KINDS)], n, seed + i))
    for k in SYNTH_KINDS:
        items.append(synth(k, 5000 + 77 * len(k), seed))
    rng.shuffle(items)
    return items


def encode_all(torch, ctx, items, fmt, lvl, P):
    keep = [dev(torch, d) for d in items]
    caps = [zz.bound(len(d), fmt, lvl, P) for d in items]
    dsts = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    lens = ctx.encode_batch([(t.data_ptr(), len(d)) for t, d in zip(keep, items)], dsts, fmt, lvl, P)
    assert None not in lens
    return [(t.data_ptr(), n) for t, n in zip(dsts, lens)], dsts


def decode_streams(torch, ctx, streams, fmt, caps):
    """streams: bytes each in its own exact allocation; destinations of caps[i] + GUARD bytes filled with 0xEE.
    Returns (rc, lens, status, outputs as bytes including the guard)."""
    keep = [dev(torch, s) for s in streams]
    outs = [torch.full((c + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    lens, status = ctx.decode_batch([(t.data_ptr(), len(s)) for t, s in zip(keep, streams)],
                                    [(t.data_ptr(), c) for t, c in zip(outs, caps)], fmt)
    torch.cuda.synchronize()
    return lens, status, [t.cpu().numpy().tobytes() for t in outs]


@pytest.mark.parametrize("P", [32768, 4096, 1000])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_round_trip_of_encode_batch(torch, ctx, corpus, lvl, P):
    items = item_set(corpus, P, 17 * lvl + P)
    for fmt in range(3):
        srcs, keep = encode_all(torch, ctx, items, fmt, lvl, P)
        outs = [torch.full((len(d) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for d in items]
        lens, status = ctx.decode_batch(srcs, [(t.data_ptr(), len(d)) for t, d in zip(outs, items)], fmt)
        assert status == [0] * len(items)
        for i, d in enumerate(items):
            assert lens[i] == len(d), (i, fmt)
            got = outs[i].cpu().numpy().tobytes()
            assert got[: len(d)] == d, (i, len(d), fmt)
            assert got[len(d):] == b"\xEE" * GUARD
        # the same bytes and lengths as one decode call per item, on all three paths of the single decoder
        for i in range(0, len(items), 4):
            d = items[i]
            for path, (ps, idx) in enumerate(((P, None), (0, None), (P, "index"))):
                if idx and not d:
                    continue
                if idx:
                    src = dev(torch, d)
                    one = torch.zeros(zz.bound(len(d), fmt, lvl, P), dtype=torch.uint8, device="cuda")
                    w = ctx.encode(src, len(d), one, one.numel(), fmt, lvl, P)
                    index = ctx.packet_index()
                    out = torch.zeros(len(d) + 1, dtype=torch.uint8, device="cuda")
                    n = ctx.decode(one, w, out, len(d), fmt, P, index)
                else:
                    out = torch.zeros(len(d) + 1, dtype=torch.uint8, device="cuda")
                    n = ctx.decode(srcs[i][0], srcs[i][1], out, len(d), fmt, ps)
                assert n == lens[i] and out[:n].cpu().numpy().tobytes() == outs[i][:n].cpu().numpy().tobytes(), (i, path)


def test_streams_the_batch_encoder_cannot_write(torch, ctx, corpus):
    data = corpus["lcet10.txt"][:200000] + corpus["kennedy.xls"][:100000]
    src = dev(torch, data)
    for fmt in range(3):
        streams, wants = [], []

        def add(s, d):
            assert zlib.decompressobj(WBITS[fmt]).decompress(s) == d      # what zlib says the stream holds
            streams.append(s); wants.append(d)
        cap = zz.bound(len(data), fmt, 3, 1000) + 4096
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        c2 = zz.Context(0)
        c2.set_warm_window(32768)
        c2.set_extended_levels(True)
        for lvl, P in ((1, 4096), (2, 32768), (3, 1000), (4, 32768), (5, 4096), (6, 32768)):
            w = c2.encode(src, len(data), dst, cap, fmt, lvl, P)
            add(dst[:w].cpu().numpy().tobytes(), data)
        c2.close()
        for lvl in (0, 1, 2, 3):
            w = ctx.encode_stream(src, len(data), dst, cap, fmt, lvl)
            add(dst[:w].cpu().numpy().tobytes(), data)
        for lvl in (0, 2, 3):
            w = ctx.encode_ranges(src, len(data), dst, cap, 7, fmt, lvl)
            add(dst[:w].cpu().numpy().tobytes(), data)
        for lvl in (0, 1, 6, 9):
            co = zlib.compressobj(lvl, zlib.DEFLATED, WBITS[fmt])
            add(co.compress(data) + co.flush(), data)
            small = corpus["xargs.1"]
            co = zlib.compressobj(lvl, zlib.DEFLATED, WBITS[fmt])
            add(co.compress(small) + co.flush(), small)
        if fmt == 1:
            add(gzip.compress(data), data)
            h = b"\x1f\x8b\x08\x1c\x00\x00\x00\x00\x00\x03" + b"\x04\x00abcd" + b"name\x00" + b"comment\x00"
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            add(h + co.compress(data) + co.flush() + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little"), data)
        lens, status, outs = decode_streams(torch, ctx, streams, fmt, [len(d) for d in wants])
        assert status == [0] * len(streams)
        for i, d in enumerate(wants):
            assert lens[i] == len(d) and outs[i] == d + b"\xEE" * GUARD, (fmt, i)


def raw_call(torch, ctx, streams, fmt, caps, with_status=True):
    keep = [dev(torch, s) for s in streams]
    outs = [torch.full((c + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for c in caps]
    table = torch.tensor([[t.data_ptr() for t in keep], [len(s) for s in streams], [t.data_ptr() for t in outs], caps],
                         dtype=torch.int64).cuda()
    lens = torch.full((len(streams),), 7, dtype=torch.int64, device="cuda")
    status = torch.full((len(streams),), 7, dtype=torch.int32, device="cuda")
    rc = zz.lib.zz_decode_batch_device(ctx._h, len(streams), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                       table[3].data_ptr(), lens.data_ptr(), status.data_ptr() if with_status else None, fmt, None)
    torch.cuda.synchronize()
    return rc, lens.cpu().tolist(), status.cpu().tolist(), [t.cpu().numpy().tobytes() for t in outs]


@pytest.mark.parametrize("fmt", [0, 1])
def test_mixed_batch_every_item_its_own_status(torch, ctx, corpus, fmt):
    good = [corpus[f][:20000] for f in CORPUS_FILES] + [synth(k, 7000, 5) for k in SYNTH_KINDS]

    def comp(d, lvl=6):
        co = zlib.compressobj(lvl, zlib.DEFLATED, WBITS[fmt])
        return co.compress(d) + co.flush()
    victim = corpus["fields.c"]
    s = comp(victim)
    flipped = bytearray(s); flipped[len(s) // 2] ^= 0x10
    assert_bad = False
    try:
        zlib.decompressobj(WBITS[fmt]).decompress(bytes(flipped))
    except zlib.error:
        assert_bad = True
    assert assert_bad, "the flipped bit must make a stream zlib refuses too"
    trailer = bytearray(s); trailer[-1] ^= 1
    fdict = b"\x78\xbb" + s[2:] if fmt == 0 else None
    bad = [("truncated", s[: len(s) - 9], len(victim), zz.E_DATA), ("flipped", bytes(flipped), len(victim) + 4096, zz.E_DATA),
           ("trailer", bytes(trailer), len(victim), zz.E_DATA), ("short cap", s, len(victim) - 1, zz.E_NOSPACE),
           ("empty item", b"", 16, zz.E_DATA), ("behind trailer", s + b"\x00", len(victim), zz.E_DATA)]
    if fdict:
        bad.append(("fdict", fdict, len(victim), zz.E_UNSUPPORTED))
    streams, caps, want = [], [], []
    for i, d in enumerate(good):
        streams.append(comp(d, (1, 6, 9)[i % 3])); caps.append(len(d) + (i % 2)); want.append((0, d))
        if i < len(bad):
            streams.append(bad[i][1]); caps.append(bad[i][2]); want.append((bad[i][3], None))
    rc, lens, status, outs = raw_call(torch, ctx, streams, fmt, caps)
    assert rc == zz.E_DATA
    for i, (st, d) in enumerate(want):
        assert status[i] == st, (i, status[i], st)
        assert outs[i][caps[i]:] == b"\xEE" * GUARD, i
        if st == 0:
            assert lens[i] == len(d) and outs[i][: len(d)] == d
        else:
            assert lens[i] == -1
    # only no-space failures: ZZ_E_NOSPACE; all good: ZZ_OK; d_status may be NULL
    only = [comp(d) for d in good]
    caps = [len(d) - (1 if i % 4 == 1 else 0) for i, d in enumerate(good)]
    rc, lens, status, outs = raw_call(torch, ctx, only, fmt, caps)
    assert rc == zz.E_NOSPACE
    assert status == [zz.E_NOSPACE if i % 4 == 1 else 0 for i in range(len(good))]
    assert all(outs[i][caps[i]:] == b"\xEE" * GUARD for i in range(len(good)))
    rc, lens, status, outs = raw_call(torch, ctx, only, fmt, [len(d) for d in good], with_status=False)
    assert rc == 0 and status == [7] * len(good) and lens == [len(d) for d in good]
    assert all(outs[i][: len(d)] == d for i, d in enumerate(good))
    # with a data failure and a no-space failure in one batch the data failure decides
    rc, _, status, _ = raw_call(torch, ctx, [only[0], s[:-5], only[1]], fmt, [len(good[0]) - 1, len(victim), len(good[1])])
    assert rc == zz.E_DATA and status == [zz.E_NOSPACE, zz.E_DATA, 0]


def test_arguments(torch, ctx):
    L = zz.lib
    assert L.zz_decode_batch_device(ctx._h, 0, None, None, None, None, None, None, 0, None) == 0
    assert ctx.decode_batch([], []) == ([], [])
    t = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    assert L.zz_decode_batch_device(ctx._h, 1, None, p, p, p, p, None, 0, None) == -4
    assert L.zz_decode_batch_device(ctx._h, 1, p, p, p, p, None, None, 0, None) == -4
    assert L.zz_decode_batch_device(ctx._h, 1, p, p, p, p, p, None, 3, None) == -4
    assert L.zz_decode_batch_device(ctx._h, 1, p, p, p, p, p, None, -1, None) == -4
    assert L.zz_decode_batch_device(ctx._h, 1 << 31, p, p, p, p, p, None, 0, None) == -4
    with pytest.raises(ValueError):
        ctx.decode_batch([t.view(torch.uint8)], [])
    with pytest.raises(TypeError):
        ctx.decode_batch([t], [t])


def test_layouts(torch, ctx, corpus):
    big = corpus["lcet10.txt"] + corpus["kennedy.xls"][:200000]
    rng = random.Random(4)
    cuts = [(rng.randrange(0, len(big) - 70000) | 1, rng.choice([0, 1, 7, 4095, 4097, 65537])) for _ in range(40)]
    items = [big[o:o + n] for o, n in cuts]
    for fmt in range(3):
        streams = []
        for i, d in enumerate(items):
            co = zlib.compressobj((1, 6, 9)[i % 3], zlib.DEFLATED, WBITS[fmt])
            streams.append(co.compress(d) + co.flush())
        # sources back to back behind one odd byte, destinations at odd offsets with a guard byte between them
        blob = b"\x55" + b"".join(streams)
        t = dev(torch, blob)
        soff, doff, a, b = [], [], 1, 1
        for s, d in zip(streams, items):
            soff.append(a); a += len(s)
            doff.append(b); b += len(d) + 1 + (len(d) % 2 == 0)      # keeps every offset odd
        out = torch.full((b + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        lens, status = ctx.decode_batch([(t.data_ptr() + o, len(s)) for o, s in zip(soff, streams)],
                                        [(out.data_ptr() + o, len(d)) for o, d in zip(doff, items)], fmt)
        host = out.cpu().numpy().tobytes()
        assert status == [0] * len(items) and lens == [len(d) for d in items]
        want = bytearray(b"\xEE" * len(host))
        for o, d in zip(doff, items):
            want[o:o + len(d)] = d
        assert host == bytes(want)
        # separate exact-size allocations
        lens, status, outs = decode_streams(torch, ctx, streams, fmt, [len(d) for d in items])
        assert status == [0] * len(items)
        assert all(o == d + b"\xEE" * GUARD for o, d in zip(outs, items))


def test_last_call_state_is_left_alone(torch, ctx, corpus):
    d = corpus["alice29.txt"]
    src = dev(torch, d)
    cap = zz.bound(len(d), 0, 2, 4096)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, len(d), dst, cap, 0, 2, 4096)
    out = torch.zeros(len(d), dtype=torch.uint8, device="cuda")
    assert ctx.decode(dst, w, out, len(d), 0, 4096) == len(d)
    before = (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.verify_last(), ctx.packet_index().cpu().tolist())
    assert before[0] == zz.DECODE_DISCOVERED
    disc = ctx.last_decode_index().cpu().tolist()
    lens, status, outs = decode_streams(torch, ctx, [zlib.compress(d), b"junk"], 0, [len(d), 10])
    assert status == [0, zz.E_DATA] and outs[0][: len(d)] == d
    after = (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.verify_last(), ctx.packet_index().cpu().tolist())
    assert after == before
    assert ctx.last_decode_index().cpu().tolist() == disc


def compare_on_device(torch, outs, want):
    return bool(torch.equal(outs, want))


def test_scale_262144_items_of_4_kib(torch, ctx):
    n, sz = 262144, 4096
    src = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_MIX, 3, 0, src, n * sz)
    cap = zz.bound(sz, 0, 1, 4096)
    comp = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    sp, cp = src.data_ptr(), comp.data_ptr()
    lens = ctx.encode_batch([(sp + i * sz, sz) for i in range(n)], [(cp + i * cap, cap) for i in range(n)], 0, 1, 4096)
    out = torch.full((n * sz + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    op = out.data_ptr()
    dl, status = ctx.decode_batch([(cp + i * cap, lens[i]) for i in range(n)], [(op + i * sz, sz) for i in range(n)], 0)
    assert dl == [sz] * n and not any(status)
    assert torch.equal(out[: n * sz], src) and bool((out[n * sz:] == 0xEE).all())


def test_scale_a_million_tiny_items(torch, ctx):
    n = 1000000
    rng = random.Random(8)
    sizes = [rng.randint(1, 64) for _ in range(n)]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    total = offs[-1]
    src = torch.empty((total + 65535) // 65536 * 65536, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 9, 0, src, src.numel())
    cap = zz.bound(64, 1, 2, 32768)
    comp = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    sp, cp = src.data_ptr(), comp.data_ptr()
    lens = ctx.encode_batch([(sp + offs[i], sizes[i]) for i in range(n)], [(cp + i * cap, cap) for i in range(n)], 1, 2, 32768)
    assert None not in lens
    out = torch.full((total + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    op = out.data_ptr()
    dl, status = ctx.decode_batch([(cp + i * cap, lens[i]) for i in range(n)], [(op + offs[i], sizes[i]) for i in range(n)], 1)
    assert dl == sizes and not any(status)
    assert torch.equal(out[:total], src[:total]) and bool((out[total:] == 0xEE).all())


def test_one_large_item_among_small_ones(torch, ctx):
    big_n, n, sz = 16 << 20, 5000, 3000
    src = torch.empty(big_n + (n * sz + 65535) // 65536 * 65536, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_LOG, 2, 0, src, src.numel())
    items = [(big_n + i * sz, sz) for i in range(n)]
    items.insert(2500, (0, big_n))
    caps = [zz.bound(ln, 0, 1, 32768) for _, ln in items]
    coff = [0]
    for c in caps:
        coff.append(coff[-1] + c)
    comp = torch.empty(coff[-1], dtype=torch.uint8, device="cuda")
    sp, cp = src.data_ptr(), comp.data_ptr()
    lens = ctx.encode_batch([(sp + o, ln) for o, ln in items], [(cp + coff[i], caps[i]) for i in range(len(items))], 0, 1, 32768)
    out = torch.full((src.numel() + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    op = out.data_ptr()
    dl, status = ctx.decode_batch([(cp + coff[i], lens[i]) for i in range(len(items))], [(op + o, ln) for o, ln in items], 0)
    assert dl == [ln for _, ln in items] and not any(status)
    used = big_n + n * sz
    assert torch.equal(out[:used], src[:used]) and bool((out[used:] == 0xEE).all())
