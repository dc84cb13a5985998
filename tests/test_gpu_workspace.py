"""A context's buffers are shared between the call kinds, which size them by different rules (packets x stride, a stream's
bound, ranges x bound, a batch's slot total ...): every call kind on ONE context, small after large and large after small, writes
what it writes on a fresh context; the workspace only grows, and grows the same way twice; contexts come and go.
Needs a real MI355X: run with `-m gpu`."""
import pytest

import zzflate_amd as zz

pytestmark = pytest.mark.gpu
ZLIB, GZIP = zz.Format.Zlib, zz.Format.Gzip
BATCH_SIZES = [0, 1, 4095, 4097, 70000]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def text():
    return zz.generate_host(zz.GEN_TEXT, 0x5EED0007, 0, 600000)


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def encode(torch, ctx, d, fmt, lvl, P=zz.DEFAULT_PACKET):
    cap = zz.bound(len(d), fmt, lvl, P)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(dev(torch, d), len(d), dst, cap, fmt, lvl, P)
    return dst[:w].cpu().numpy().tobytes()


def encode_batch(torch, ctx, items, fmt, lvl, P=zz.DEFAULT_PACKET):
    srcs = [dev(torch, d) for d in items]
    caps = [zz.bound(len(d), fmt, lvl, P) for d in items]
    dsts = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    lens = ctx.encode_batch([(t.data_ptr(), len(d)) for t, d in zip(srcs, items)], dsts, fmt, lvl, P)
    torch.cuda.synchronize()
    assert None not in lens
    return [t[:w].cpu().numpy().tobytes() for t, w in zip(dsts, lens)]


def encode_stream(torch, ctx, d, lvl):
    cap = 2 * len(d) + 1024
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode_stream(dev(torch, d), len(d), dst, cap, ZLIB, lvl)
    return dst[:w].cpu().numpy().tobytes()


def encode_ranges(torch, ctx, d, lvl, count):
    cap = 2 * len(d) + 1024
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode_ranges(dev(torch, d), len(d), dst, cap, count, ZLIB, lvl)
    return dst[:w].cpu().numpy().tobytes()


def encode_members(torch, ctx, d, lvl):
    cap = zz.members_bound(len(d))
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode_members(dev(torch, d), len(d), dst, cap, level=lvl)
    return dst[:w].cpu().numpy().tobytes()


def decode(torch, ctx, s, n):
    dst = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    w = ctx.decode(dev(torch, s), len(s), dst, n + 1, ZLIB)
    return dst[:w].cpu().numpy().tobytes()


def decode_batch(torch, ctx, streams, sizes):
    srcs = [dev(torch, s) for s in streams]
    dsts = [torch.zeros(n + 1, dtype=torch.uint8, device="cuda") for n in sizes]
    lens, status = ctx.decode_batch(srcs, dsts, ZLIB)
    torch.cuda.synchronize()
    assert status == [0] * len(streams)
    return [t[:w].cpu().numpy().tobytes() for t, w in zip(dsts, lens)]


def steps(torch, text):
    """the sequence: (name, call(ctx, outputs of the earlier steps by name) -> what the step wrote)"""
    items = [text[100000:100000 + n] for n in BATCH_SIZES]
    return [
        ("encode_l2", lambda c, o: encode(torch, c, text[:300000], ZLIB, 2, 4096)),
        ("batch_l1", lambda c, o: encode_batch(torch, c, items, ZLIB, 1)),
        ("members_l1", lambda c, o: encode_members(torch, c, text[:200000], 1)),   # on item buffers the larger batch has grown
        ("batch_l2_gzip", lambda c, o: encode_batch(torch, c, items, GZIP, 2)),     # and a batch on what members left there
        ("stream_l2", lambda c, o: encode_stream(torch, c, text[:100000], 2)),
        ("ranges_l2", lambda c, o: encode_ranges(torch, c, text[:200000], 2, 3)),
        ("encode_l1_gzip", lambda c, o: encode(torch, c, text[:1000], GZIP, 1)),
        ("encode_l3", lambda c, o: encode(torch, c, text, ZLIB, 3)),          # every shared buffer grows after smaller uses
        ("decode", lambda c, o: decode(torch, c, o["encode_l3"], len(text))),
        ("decode_batch", lambda c, o: decode_batch(torch, c, o["batch_l1"], BATCH_SIZES)),
    ]


def run_sequence(torch, text):
    """all steps on one context: their outputs, and the workspace's size before the first step and after every one"""
    ctx = zz.Context(0)
    out, ws = {}, [ctx.workspace_bytes()]
    for name, call in steps(torch, text):
        out[name] = call(ctx, out)
        ws.append(ctx.workspace_bytes())
    ctx.close()
    return out, ws


@pytest.fixture(scope="module")
def shared(torch, text):
    return run_sequence(torch, text)


def test_shared_buffers_write_what_a_fresh_context_writes(torch, text, shared):
    out, _ = shared
    for name, call in steps(torch, text):
        fresh = zz.Context(0)
        alone = call(fresh, out)
        fresh.close()
        assert out[name] == alone, name
    assert out["decode"] == text
    assert out["decode_batch"] == [text[100000:100000 + n] for n in BATCH_SIZES]


def test_workspace_only_grows_and_grows_the_same_way_twice(torch, text, shared):
    _, ws = shared
    assert all(b >= a for a, b in zip(ws, ws[1:])), ws
    assert ws[-1] > ws[0]
    _, again = run_sequence(torch, text)
    assert again[-1] == ws[-1], (ws, again)


def test_contexts_come_and_go(torch, text):
    d, items = text[:4096], [text[5000:9000], text[9000:9001]]
    want = None
    for _ in range(20):
        ctx = zz.Context(0)
        got = (encode(torch, ctx, d, ZLIB, 1), encode_batch(torch, ctx, items, ZLIB, 1))
        ctx.close()
        want = want or got
        assert got == want
