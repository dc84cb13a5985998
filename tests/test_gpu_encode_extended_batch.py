"""Levels 4..6 of zz_encode_batch_flags_device (ZZ_BATCH_EXTENDED) and zz_encode_members_device (ZZ_MEMBERS_EXTENDED): every item
and every member is, byte for byte, the oracle's stream of its own bytes alone (tests/extended_batch_cases.py) -- whatever lies
in front of it in memory --, across the packet and block edges, through several rounds of the match words and the work counter,
with destinations that are too small, and the refusals. Needs a real MI355X: run with `-m gpu`."""
import ctypes
import gzip
import os
import subprocess
import sys
import tempfile

import pytest

import zzflate_amd as zz
import extended_batch_cases as xc
import members_write_cases as mw
from conftest import ROOT

pytestmark = pytest.mark.gpu
ERR = (1 << 64) - 1
E_LEVEL = -1
GUARD = 96


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


@pytest.fixture(scope="module")
def on_device(torch):
    """items(P) on the device, uploaded once per packet size"""
    return {P: [dev(torch, d) for d in xc.items(P)] for P in xc.PACKETS}


def batch(torch, ctx, srcs, sizes, fmt, level, P):
    """one switched call; (lens, destinations): destinations of zz.bound bytes with zeros behind them"""
    caps = [zz.bound(n, fmt, 2, P) for n in sizes]
    dsts = [torch.zeros(c + 64, dtype=torch.uint8, device="cuda") for c in caps]
    lens = ctx.encode_batch_extended(srcs, [(t.data_ptr(), c) for t, c in zip(dsts, caps)], fmt, level, P, caps=caps)
    torch.cuda.synchronize()
    return lens, dsts


@pytest.mark.parametrize("P", xc.PACKETS)
@pytest.mark.parametrize("level", xc.LEVELS)
@pytest.mark.parametrize("fmt", xc.FORMATS)
def test_batch_bytes(torch, ctx, oracle, on_device, fmt, level, P):
    items, want = xc.items(P), xc.expected_items(oracle, fmt, level, P)
    keep = on_device[P]
    lens, dsts = batch(torch, ctx, [(t.data_ptr(), len(d)) for t, d in zip(keep, items)], [len(d) for d in items], fmt, level, P)
    for i, d in enumerate(items):
        assert lens[i] == len(want[i]), (i, len(d))
        assert dsts[i][: lens[i]].cpu().numpy().tobytes() == want[i], (i, len(d))
        assert dsts[i][lens[i]:].count_nonzero().item() == 0, i               # nothing written behind the stream
    outs = [torch.zeros(len(d) + 1, dtype=torch.uint8, device="cuda") for d in items]
    back, status = ctx.decode_batch([(t.data_ptr(), n) for t, n in zip(dsts, lens)], outs, fmt)
    assert status == [0] * len(items) and back == [len(d) for d in items]
    for o, d in zip(outs, items):
        assert o[: len(d)].cpu().numpy().tobytes() == d


@pytest.mark.parametrize("level", xc.LEVELS)
def test_a_copy_in_front_of_an_item_is_not_its_window(torch, ctx, oracle, level):
    for name, X in xc.copy_cases():
        buf = dev(torch, X * 3)
        want = oracle.encode_packets(X, xc.DEFLATE, level)
        lens, dsts = batch(torch, ctx, [(buf.data_ptr() + i * xc.COPY, xc.COPY) for i in range(3)], [xc.COPY] * 3, xc.DEFLATE, level, 32768)
        for i in range(3):
            assert dsts[i][: lens[i]].cpu().numpy().tobytes() == want, (name, i)


@pytest.mark.parametrize("level", xc.LEVELS)
def test_a_copy_in_front_of_a_block_is_not_its_window(torch, ctx, oracle, level):
    for name, X in xc.copy_cases():
        data = X * 3
        want, offsets, stored = mw.expected(oracle, data, level, xc.COPY, mw.PACKET, True)
        alone = oracle.encode_packets(X, xc.DEFLATE, level)
        cap = zz.members_bound(len(data), xc.COPY, mw.PACKET)
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        w = ctx.encode_members_extended(dev(torch, data), len(data), dst, cap, level, xc.COPY, mw.PACKET)
        file = dst[:w].cpu().numpy().tobytes()
        assert file == want, name
        for at, size in mw.members_of(file[:offsets[-1]]):
            assert file[at + 18:at + size - 8] == alone, (name, at)              # every member: the stream of X alone
        assert gzip.decompress(file) == data


CHILD = r"""
import sys
import torch
import zzflate_amd as zz
sizes = [int(v) for v in open(sys.argv[1] + ".sizes").read().split()]
data = open(sys.argv[1] + ".in", "rb").read()
buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
offs = [0]
for n in sizes:
    offs.append(offs[-1] + n)
ctx = zz.Context(0)
with open(sys.argv[1] + ".out", "wb") as f:
    for level in (4, 5, 6):
        caps = [zz.bound(n, 2, 2, 4096) for n in sizes]
        dsts = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
        lens = ctx.encode_batch_extended([(buf.data_ptr() + o, n) for o, n in zip(offs, sizes)], [(t.data_ptr(), c) for t, c in zip(dsts, caps)],
                                         2, level, 4096, caps=caps)
        torch.cuda.synchronize()
        for t, ln in zip(dsts, lens):
            f.write(ln.to_bytes(4, "little") + t[:ln].cpu().numpy().tobytes())
ctx.close()
"""


def test_rounds_and_the_work_counter(oracle):
    """1 MiB of match words per round = 256 packets of 4,096 bytes, three match workgroups: the 700 items make at least three rounds,
    the last one not full, every round with more packets than workgroups (the two variables are read once per process: a child)"""
    items = xc.many_items()
    P, per_round, wgs = 4096, (1 << 20) // 4096, 3
    npk = sum(-(-len(d) // P) for d in items)
    assert npk > 2 * per_round and wgs < npk % per_round < per_round
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "rounds")
        open(base + ".in", "wb").write(b"".join(items))
        open(base + ".sizes", "w").write(" ".join(str(len(d)) for d in items))
        env = dict(os.environ, ZZFLATE_L6_BATCH_MIB="1", ZZFLATE_L6_MATCH_WGS=str(wgs), PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", CHILD, base], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        out = open(base + ".out", "rb").read()
    at = 0
    for level in xc.LEVELS:
        for i, d in enumerate(items):
            ln = int.from_bytes(out[at:at + 4], "little")
            assert out[at + 4:at + 4 + ln] == oracle.encode_packets(d, xc.DEFLATE, level, P), (level, i, len(d))
            at += 4 + ln
    assert at == len(out)


@pytest.mark.parametrize("level", xc.LEVELS)
def test_a_destination_one_byte_short(torch, ctx, oracle, on_device, level):
    P, fmt = 4096, xc.GZIP
    items, want, keep = xc.items(P), xc.expected_items(oracle, fmt, level, P), on_device[P]
    short = len(xc.lengths(P)) - 1                                             # the item of 3P + 5 bytes
    caps = [len(w) - (1 if i == short else 0) for i, w in enumerate(want)]
    dsts = [torch.full((c + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for c in caps]
    table = torch.tensor([[k.data_ptr() for k in keep], [len(d) for d in items], [t.data_ptr() for t in dsts], caps], dtype=torch.int64).cuda()
    outl = torch.zeros(len(items), dtype=torch.int64, device="cuda")
    rc = zz.lib.zz_encode_batch_flags_device(ctx._h, len(items), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                             table[3].data_ptr(), outl.data_ptr(), fmt, level, P, zz.BATCH_EXTENDED,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == zz.E_NOSPACE
    lens = [v & ERR for v in outl.cpu().tolist()]
    for i in range(len(items)):
        host = dsts[i].cpu().numpy().tobytes()
        assert host[caps[i]:] == b"\xa5" * GUARD, i                              # guard bytes behind every cap
        if i == short:
            assert lens[i] == ERR
        else:
            assert lens[i] == len(want[i]) and host[: lens[i]] == want[i], i     # every other item is complete


def write(torch, ctx, data, level, B, P, eof, cap=None):
    src = dev(torch, data)
    cap = zz.members_bound(len(data), B, P, eof) if cap is None else cap
    dst = torch.zeros(cap + GUARD, dtype=torch.uint8, device="cuda")
    members = -(-len(data) // B)
    offs = torch.full((members + 1,), -1, dtype=torch.int64, device="cuda")
    w = ctx.encode_members_extended(src, len(data), dst, cap, level, B, P, eof, offs)
    torch.cuda.synchronize()
    raw = dst.cpu().numpy().tobytes()
    return raw[:w], raw[w:], offs.cpu().tolist(), ctx.last_encode_members_stats()


@pytest.mark.parametrize("level", xc.LEVELS)
def test_members_byte_for_byte_and_round_trip(torch, ctx, oracle, level):
    for index, (name, data, B, P, eof) in enumerate(mw.cases(oracle)):
        want, offsets, stored = mw.expected_case(oracle, index, level)
        file, behind, offs, stats = write(torch, ctx, data, level, B, P, eof)
        assert file == want, (name, len(file), len(want))
        assert behind == bytes(len(behind)), name
        assert offs == offsets, name
        assert stats == (len(stored), sum(stored)), name
        if file:
            assert gzip.decompress(file) == data, name
            out = torch.zeros(len(data) + 1, dtype=torch.uint8, device="cuda")
            w = ctx.decode_members(dev(torch, file), len(file), out, len(data) + 1)
            assert out[:w].cpu().numpy().tobytes() == data, name
            if b"\x1f\x8b\x08" not in data:
                assert ctx.last_decode_members_stats()[2] == zz.MEMBERS_BLOCKED == 1, name


@pytest.mark.parametrize("level", xc.LEVELS)
def test_members_one_byte_short_writes_nothing(torch, ctx, oracle, level):
    data = mw.mixed(40000, 100000, 60000, 2)
    want = mw.expected(oracle, data, level, mw.BLOCK, mw.PACKET, True)[0]
    src = dev(torch, data)
    cap = len(want) - 1
    dst = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = ctypes.c_uint64(0)
    rc = zz.lib.zz_encode_members_device(ctx._h, src.data_ptr(), len(data), dst.data_ptr(), cap, ctypes.byref(out), level, 0, 0,
                                         zz.MEMBERS_EXTENDED, None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (rc, out.value) == (zz.E_NOSPACE, ERR)
    assert dst.cpu().numpy().tobytes() == b"\xa5" * (cap + GUARD)
    assert ctx.last_encode_members_stats() == (0, 0)
    assert write(torch, ctx, data, level, mw.BLOCK, mw.PACKET, True, cap=len(want))[0] == want   # exactly enough room


def test_refusals_and_state(torch, oracle):
    data = mw.text(70000, 4)
    src = dev(torch, data)
    out = torch.zeros(zz.bound(len(data), 0, 2) + 64, dtype=torch.uint8, device="cuda")
    mdst = torch.zeros(zz.members_bound(len(data)), dtype=torch.uint8, device="cuda")
    c = zz.Context(0)

    def code(fn, *a, **k):
        with pytest.raises(zz.ZzFlateError) as e:
            fn(*a, **k)
        return e.value.code

    def batch_x(level):
        return c.encode_batch_extended([src], [out], zz.Format.Zlib, level)

    def members_x(level):
        return c.encode_members_extended(src, len(data), mdst, mdst.numel(), level)

    try:
        # without the switch nothing has changed
        assert code(c.encode_batch, [src], [out], level=4) == E_LEVEL
        assert code(c.encode_members, src, len(data), mdst, mdst.numel(), 4) == E_LEVEL
        # a warm window refuses, whatever the level
        c.set_warm_window(4096)
        for level in (1, 6):
            assert code(batch_x, level) == zz.E_UNSUPPORTED and code(members_x, level) == zz.E_UNSUPPORTED
        c.set_warm_window(0)
        for level in (-1, 7):
            assert code(batch_x, level) == E_LEVEL and code(members_x, level) == E_LEVEL
        unknown = zz.lib.zz_encode_batch_flags_device(c._h, 1, None, None, None, None, None, 0, 6, 0, 2, None)
        assert unknown == zz.E_ARG
        # a device whose LDS-order verdict is negative: levels 4..6 refuse, level 2 works
        zz.lib.zz_debug_force_lds_order(0)
        assert code(batch_x, 6) == zz.E_UNSUPPORTED and b"extended levels refused" in zz.lib.zz_last_error()
        assert code(members_x, 6) == zz.E_UNSUPPORTED
        w = batch_x(2)[0]
        assert out[:w].cpu().numpy().tobytes() == oracle.encode_packets(data, 0, 2)
        assert members_x(2) == len(mw.expected(oracle, data, 2, mw.BLOCK, mw.PACKET, True)[0])
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_reset_lds_order(0)
        # the switch is the call's: the context's own does not matter and does not move
        c.set_extended_levels(True)
        w = batch_x(6)[0]
        assert out[:w].cpu().numpy().tobytes() == oracle.encode_packets(data, 0, 6)
        assert batch_x(1)[0] == len(oracle.encode_packets(data, 0, 1))
        c.set_extended_levels(False)
        w = batch_x(6)[0]
        assert out[:w].cpu().numpy().tobytes() == oracle.encode_packets(data, 0, 6)
        dst = torch.zeros(zz.bound(len(data), 0, 2), dtype=torch.uint8, device="cuda")
        assert code(c.encode, src, len(data), dst, dst.numel(), zz.Format.Zlib, 6) == E_LEVEL
        # a switched call is not the context's last call
        c.encode(src, len(data), dst, dst.numel(), zz.Format.Zlib, 1)
        assert c.verify_last() == (0, None)
        batch_x(5)
        bad = ctypes.c_uint64(0)
        assert zz.lib.zz_verify_last_device(c._h, ctypes.byref(bad), ctypes.byref(bad), None) == zz.E_ARG
        c.encode(src, len(data), dst, dst.numel(), zz.Format.Zlib, 1)
        assert members_x(4) == len(mw.expected(oracle, data, 4, mw.BLOCK, mw.PACKET, True)[0])
        assert zz.lib.zz_verify_last_device(c._h, ctypes.byref(bad), ctypes.byref(bad), None) == zz.E_ARG
        # the timed work covers both kernels of the extended levels
        c.enable_timing(True)
        batch_x(6)
        assert c.last_kernel_ms() > 0
        c.enable_timing(False)
    finally:
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_reset_lds_order(0)
        c.close()
