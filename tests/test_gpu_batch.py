"""zz_encode_batch_device / Context.encode_batch: many independent streams in one call. Every item's stream equals the single call
on that item alone (ctx.encode) and the oracle's, whatever the layout of sources and destinations; items that do not fit are
reported and leave the others complete. Needs a real MI355X: run with `-m gpu`."""
import ctypes
import random
import zlib

import pytest

import zzflate_amd as zz
from conftest import CORPUS_FILES, SYNTH_KINDS, synth

pytestmark = pytest.mark.gpu
WBITS = {0: 15, 1: 31, 2: -15}
LEVELS = [0, 1, 2, 3]
ERR = (1 << 64) - 1


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


def dev(torch, b):
    """b on the device in an allocation of exactly len(b) bytes (one byte for an empty item: never read)"""
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def single(torch, ctx, d, fmt, lvl, P):
    src = dev(torch, d)
    cap = zz.bound(len(d), fmt, lvl, P)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, len(d), dst, cap, fmt, lvl, P)
    return dst[:w].cpu().numpy().tobytes()


def batch(torch, ctx, items, fmt, lvl, P, caps=None):
    """items in their own exactly-sized allocations, destinations of zz.bound bytes (or caps)"""
    keep = [dev(torch, d) for d in items]
    srcs = [(t.data_ptr(), len(d)) for t, d in zip(keep, items)]
    caps = caps or [zz.bound(len(d), fmt, lvl, P) for d in items]
    dsts = [torch.zeros(c + 64, dtype=torch.uint8, device="cuda") for c in caps]
    lens = ctx.encode_batch(srcs, [(t.data_ptr(), c) for t, c in zip(dsts, caps)], fmt, lvl, P, caps=caps)
    torch.cuda.synchronize()
    return lens, dsts, keep


def item_set(corpus, P, seed):
    """the corpus, every synth family, and the sizes around the packet edges, shuffled"""
    rng = random.Random(seed)
    items = [corpus[f] for f in CORPUS_FILES]
    sizes = [0, 1, 2, 63, 64, 65, P - 1, P, P + 1, 3 * P + 7, (1 << 20) + 13]
    for i, n in enumerate(sizes):
        items.append(synth(SYNTH_KINDS[i % len(SYNTH_KINDS)], n, seed + i))
    for k in SYNTH_KINDS:
        items.append(synth(k, 5000 + 77 * len(k), seed))
    rng.shuffle(items)
    return items


@pytest.mark.parametrize("P", [32768, 4096, 1000])
@pytest.mark.parametrize("lvl", LEVELS)
def test_batch_equals_single_calls_and_oracle(torch, ctx, oracle, corpus, lvl, P):
    items = item_set(corpus, P, 17 * lvl + P)
    for fmt in range(3):
        lens, dsts, _ = batch(torch, ctx, items, fmt, lvl, P)
        for i, d in enumerate(items):
            got = dsts[i][: lens[i]].cpu().numpy().tobytes()
            assert got == single(torch, ctx, d, fmt, lvl, P), (i, len(d), fmt)
            if d:                         # (an empty input gets one empty final block: the single call's divergence D8, not the oracle's)
                assert got == oracle.encode_packets(d, fmt, lvl, P), (i, len(d), fmt)
            assert zlib.decompressobj(WBITS[fmt]).decompress(got) == d
            assert dsts[i][lens[i]:].count_nonzero().item() == 0          # nothing written behind the stream
        # the device decoder on a subset (the packet size tells it where packets start)
        for i in range(0, len(items), 5):
            d = items[i]
            out = torch.zeros(len(d) + 1, dtype=torch.uint8, device="cuda")
            w = ctx.decode(dsts[i], lens[i], out, len(d) + 1, fmt, P)
            assert w == len(d) and out[:w].cpu().numpy().tobytes() == d


def test_empty_batch_and_verify_after_a_batch(torch, ctx, corpus):
    L = zz.lib
    assert L.zz_encode_batch_device(ctx._h, 0, None, None, None, None, None, 0, 1, 32768, None) == 0
    assert ctx.encode_batch([], []) == []
    d = corpus["alice29.txt"]
    single(torch, ctx, d, 0, 1, 32768)
    assert ctx.verify_last() == (0, None)
    lens, _, _ = batch(torch, ctx, [d], 0, 1, 32768)
    assert lens[0] is not None
    out = ctypes.c_uint64(0)
    assert L.zz_verify_last_device(ctx._h, ctypes.byref(out), ctypes.byref(out), None) == -4
    assert L.zz_packet_extent_device(ctx._h, 0, ctypes.byref(out), ctypes.byref(out), None) == -4
    assert L.zz_packet_index_device(ctx._h, None, 0, ctypes.byref(out), None) == -4


@pytest.mark.parametrize("lvl", LEVELS)
def test_layouts(torch, ctx, oracle, corpus, lvl):
    P = 4096
    big = corpus["lcet10.txt"] + corpus["kennedy.xls"][:200000]
    t = dev(torch, big)
    rng = random.Random(lvl)
    # sub-slices at odd offsets of one tensor, overlapping, the same slice more than once
    cuts = [(rng.randrange(0, len(big) - 70000) | 1, rng.choice([0, 1, 7, 4095, 4097, 65537])) for _ in range(24)]
    cuts += [cuts[3]] * 3 + [(len(big) - 333, 333), (len(big) - 1, 1)]        # (the last byte of the allocation, too)
    items = [big[o:o + n] for o, n in cuts]
    fmt = lvl % 3
    caps = [zz.bound(len(d), fmt, lvl, P) for d in items]
    offs = [0]
    for c in caps:
        offs.append(offs[-1] + c)
    out = torch.zeros(offs[-1] + 64, dtype=torch.uint8, device="cuda")       # destinations back to back at zz.bound spacing
    lens = ctx.encode_batch([(t.data_ptr() + o, n) for o, n in cuts], [(out.data_ptr() + offs[i], caps[i]) for i in range(len(cuts))],
                            fmt, lvl, P)
    host = out.cpu().numpy().tobytes()
    for i, d in enumerate(items):
        got = host[offs[i]: offs[i] + lens[i]]
        if d:
            assert got == oracle.encode_packets(d, fmt, lvl, P), (i, cuts[i])
        assert got == single(torch, ctx, d, fmt, lvl, P)
        assert host[offs[i] + lens[i]: offs[i + 1]] == bytes(offs[i + 1] - offs[i] - lens[i])


@pytest.mark.parametrize("lvl", LEVELS)
def test_items_that_do_not_fit(torch, ctx, corpus, lvl):
    P = 4096
    items = [corpus[f][: 3000 + 9000 * j] for j, f in enumerate(CORPUS_FILES)] + [b"", b"x", bytes(100)]
    for fmt in range(3):
        exact = [len(single(torch, ctx, d, fmt, lvl, P)) for d in items]
        hl = {0: 2, 1: 10, 2: 0}[fmt]
        caps = []
        for i, e in enumerate(exact):
            caps.append(e - 1 if i % 3 == 0 else (max(hl - 1, 0) if i % 3 == 1 else e))
        keep = [dev(torch, d) for d in items]
        guard = 96
        dsts = [torch.full((c + guard,), 0xA5, dtype=torch.uint8, device="cuda") for c in caps]
        L = zz.lib
        table = torch.tensor([[k.data_ptr() for k in keep], [len(d) for d in items], [t.data_ptr() for t in dsts], caps],
                             dtype=torch.int64).cuda()
        outl = torch.zeros(len(items), dtype=torch.int64, device="cuda")
        rc = L.zz_encode_batch_device(ctx._h, len(items), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                      table[3].data_ptr(), outl.data_ptr(), fmt, lvl, P, torch.cuda.current_stream().cuda_stream)
        assert rc == zz.E_NOSPACE
        lens = [v & ERR for v in outl.cpu().tolist()]
        for i, d in enumerate(items):
            host = dsts[i].cpu().numpy().tobytes()
            assert host[caps[i]:] == b"\xa5" * guard, (i, fmt)                           # nothing behind cap
            if caps[i] >= exact[i]:
                assert lens[i] == exact[i] and host[: lens[i]] == single(torch, ctx, d, fmt, lvl, P)
            else:
                assert lens[i] == ERR, (i, caps[i], exact[i])
        # the same through Python: None for the items that did not fit
        got = ctx.encode_batch([(k.data_ptr(), len(d)) for k, d in zip(keep, items)], [(t.data_ptr(), c) for t, c in zip(dsts, caps)],
                               fmt, lvl, P)
        assert got == [e if c >= e else None for e, c in zip(exact, caps)]


@pytest.mark.parametrize("lvl", [1, 2])
def test_guard_paths_give_the_same_bytes(torch, ctx, corpus, lvl):
    items = [corpus[f] for f in CORPUS_FILES] + [synth("words", 70000, 3), b"", b"ab"]
    normal_lens, normal, _ = batch(torch, ctx, items, 0, lvl, 32768)
    want = [normal[i][: normal_lens[i]].cpu().numpy().tobytes() for i in range(len(items))]
    try:
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_order(0)                 # the one-parser forms
        lens, dsts, _ = batch(torch, ctx, items, 0, lvl, 32768)
        assert [dsts[i][: lens[i]].cpu().numpy().tobytes() for i in range(len(items))] == want
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_violation(1)             # the kernel reports a violation: the whole batch runs again
        lens, dsts, _ = batch(torch, ctx, items, 0, lvl, 32768)
        assert [dsts[i][: lens[i]].cpu().numpy().tobytes() for i in range(len(items))] == want
        assert zz.lib.zz_debug_lds_order_verdict(0) == 0
    finally:
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


def test_refusals(torch, corpus):
    d = corpus["xargs.1"]
    t = dev(torch, d)
    out = torch.zeros(zz.bound(len(d), 0, 3) + 64, dtype=torch.uint8, device="cuda")
    c = zz.Context(0)
    with pytest.raises(zz.ZzFlateError) as e:
        c.encode_batch([t], [out], level=4)
    assert e.value.code == -1
    c.set_warm_window(4096)
    with pytest.raises(zz.ZzFlateError) as e:
        c.encode_batch([t], [out], level=1)
    assert e.value.code == zz.E_UNSUPPORTED
    c.set_warm_window(0)
    assert c.encode_batch([t], [out], level=1)[0] is not None
    c.set_extended_levels(True)
    for lvl in (1, 6):
        with pytest.raises(zz.ZzFlateError) as e:
            c.encode_batch([t], [out], level=lvl)
        assert e.value.code == zz.E_UNSUPPORTED
    c.close()


def test_one_gib_of_32_kib_items(torch, ctx, oracle):
    n_items, size = 32768, 32768
    src = torch.empty(n_items * size, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 7, 0, src, src.numel())
    cap = zz.bound(size, 0, 1, size)
    dst = torch.zeros(n_items * cap, dtype=torch.uint8, device="cuda")
    base, dbase = src.data_ptr(), dst.data_ptr()
    lens = ctx.encode_batch([(base + i * size, size) for i in range(n_items)], [(dbase + i * cap, cap) for i in range(n_items)],
                            0, 1, size)
    assert None not in lens
    host = dst.cpu().numpy().tobytes()
    src_host = src.cpu().numpy().tobytes()
    for i in range(n_items):
        s = host[i * cap: i * cap + lens[i]]
        assert zlib.decompress(s) == src_host[i * size:(i + 1) * size], i
    for i in random.Random(5).sample(range(n_items), 24):
        d = zz.generate_host(zz.GEN_TEXT, 7, (i * size) & ~65535, 65536)[(i * size) & 65535:][:size]
        assert d == src_host[i * size:(i + 1) * size]
        assert host[i * cap: i * cap + lens[i]] == oracle.encode_packets(d, 0, 1, size), i


def test_a_million_items_in_one_call(torch, ctx):
    """1,000,000 items of 64 bytes: the five arrays are built on the device, the call takes them as they are."""
    k, size = 1000000, 64
    src = torch.empty(k * size, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_MIX, 11, 0, src, src.numel())
    for lvl in (1, 2):
        cap = zz.bound(size, 1, lvl, 32768)
        dst = torch.zeros(k * cap, dtype=torch.uint8, device="cuda")
        idx = torch.arange(k, dtype=torch.int64, device="cuda")
        srcs = src.data_ptr() + idx * size
        ns = torch.full((k,), size, dtype=torch.int64, device="cuda")
        dsts = dst.data_ptr() + idx * cap
        caps = torch.full((k,), cap, dtype=torch.int64, device="cuda")
        outl = torch.zeros(k, dtype=torch.int64, device="cuda")
        rc = zz.lib.zz_encode_batch_device(ctx._h, k, srcs.data_ptr(), ns.data_ptr(), dsts.data_ptr(), caps.data_ptr(), outl.data_ptr(),
                                           1, lvl, 32768, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, zz.lib.zz_last_error()
        lens = outl.cpu().tolist()
        assert min(lens) > 18 and max(lens) <= cap
        for i in random.Random(lvl).sample(range(k), 200):
            d = src[i * size:(i + 1) * size].cpu().numpy().tobytes()
            got = dst[i * cap: i * cap + lens[i]].cpu().numpy().tobytes()
            assert got == single(torch, ctx, d, 1, lvl, 32768), i
            assert zlib.decompress(got, 31) == d
