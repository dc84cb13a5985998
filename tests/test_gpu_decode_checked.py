"""Checked range reads on the device (zz_decode_range_checked_device, zz_decode_ranges_checked_device) and the sidecar's producer
(zz_packet_checksums_device), on the streams and damage cases of tests/checked_cases.py. Python's zlib is the yardstick: the
sidecars are zlib.adler32 / zlib.crc32 of the packets, and a damage case is one where zlib shows the packet's checksum differs.

test_damage_single_read is the test that fails without the feature: the unchecked read returns ZZ_OK and a wrong byte for the very
range the checked read refuses."""
import ctypes
import random

import pytest

from conftest import Oracle
from range_streams import ranges_for
import checked_cases as cc

torch = pytest.importorskip("torch")
import zzflate_amd as zz  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
ERR = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = zz.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def dev(data):
    return torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).cuda()[: len(data)]


def dev_cks(cks):
    return torch.tensor([v - (1 << 32) if v >> 31 else v for v in cks], dtype=torch.int32).cuda()


def patterns(t):
    return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


_on_device = {}


def on_device(t):
    """(stream, index, sidecar, decoded bytes) of an intact case stream as device tensors, made once"""
    if t.name not in _on_device:
        _on_device[t.name] = (dev(t.s), torch.tensor(t.idx, dtype=torch.int64).cuda(), dev_cks(t.cks), dev(t.data))
    return _on_device[t.name]


class Dest:
    """`room` bytes of 0xA5 between two guards, at an odd address"""

    def __init__(self, room):
        self.buf = torch.empty(room + 2 * GUARD + 1, dtype=torch.uint8, device="cuda")
        self.room = room

    def ptr(self):
        self.buf.fill_(0xA5)
        return self.buf.data_ptr() + GUARD + 1

    def got(self, n):
        return self.buf[GUARD + 1: GUARD + 1 + n]

    def untouched_outside(self, n):
        return bool((self.buf[: GUARD + 1] == 0xA5).all()) and bool((self.buf[GUARD + 1 + n:] == 0xA5).all())


def raw_checked(c, s, w, fmt, P, idx, cks, total_len, first, nbytes, p, cap):
    out = ctypes.c_uint64(5)
    rc = zz.lib.zz_decode_range_checked_device(c._h, s.data_ptr(), w, fmt, P, idx.data_ptr(), idx.numel(), cks.data_ptr(), total_len,
                                               first, nbytes, p, cap, ctypes.byref(out), c._stream())
    return rc, out.value


# ---- the producer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_producer_equals_zlib(ctx, fmt):
    rng = random.Random(fmt)
    for P in (32768, 4096, 1000, 1):
        for n in (0, 1, P - 1, P, P + 1, 3 * P + 17) if P > 1 else (0, 1, 2, 300):
            data = bytes(rng.getrandbits(8) for _ in range(n))
            got = ctx.packet_checksums(dev(data), n, fmt, P)
            assert got.dtype == torch.int32 and patterns(got) == zz.packet_checksums_host(data, fmt, P), (P, n)
    for P in (32768, 4096):                                     # all-0xFF packets (join_cases' `ff` family): Adler's sums at their largest
        data = b"\xff" * (2 * P + 5)
        assert patterns(ctx.packet_checksums(dev(data), len(data), fmt, P)) == zz.packet_checksums_host(data, fmt, P), P


def test_producer_buffer_too_small_and_state(ctx):
    data = bytes(range(256)) * 20
    src = dev(data)
    cap = zz.bound(len(data), 0, 1, 1000) + 64
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ctx.encode(src, len(data), dst, cap, 0, 1, 1000)
    before = ctx.packet_index().cpu().tolist()
    cks = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n = ctypes.c_uint64(0)
    rc = zz.lib.zz_packet_checksums_device(ctx._h, src.data_ptr(), len(data), 1000, 0, cks.data_ptr(), 5, ctypes.byref(n), ctx._stream())
    assert rc == zz.E_NOSPACE and n.value == 6 and patterns(cks) == [0x5A5A5A5A] * 8
    rc = zz.lib.zz_packet_checksums_device(ctx._h, src.data_ptr(), len(data), 1000, 0, cks.data_ptr(), 6, ctypes.byref(n), ctx._stream())
    assert rc == 0 and patterns(cks) == zz.packet_checksums_host(data, 0, 1000) + [0x5A5A5A5A] * 2
    assert ctx.packet_index().cpu().tolist() == before and ctx.verify_last()[0] == 0


# ---- intact streams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", range(6))
def test_intact_streams_every_range(ctx, oracle, part):
    for i, t in list(enumerate(cc.streams(oracle)))[part::6]:
        s, idx, cks, src = on_device(t)
        L = len(t.data)
        dest = Dest(max(L, 16))
        if L == 0:
            for first, nbytes in ((0, 5), (0, 0), (999, 3)):
                p = dest.ptr()
                assert raw_checked(ctx, s, len(t.s), t.fmt, t.P, idx, cks, 0, first, nbytes, p, 5) == (0, 0), (t.name, first)
                assert dest.untouched_outside(0)
            continue
        rs = ranges_for(L, t.P, i)
        for first, nbytes in rs:
            m = max(0, min(nbytes, L - first))
            p = dest.ptr()
            assert ctx.decode_range_checked(s, len(t.s), p, min(nbytes, dest.room), first, nbytes, cks, L, t.fmt, t.P, idx) == m, (t.name, first, nbytes)
            assert torch.equal(dest.got(m), src[first: first + m]) and dest.untouched_outside(m), (t.name, first, nbytes)
            checked_stats = ctx.last_decode_range_stats()
            p = dest.ptr()
            assert ctx.decode_range(s, len(t.s), p, min(nbytes, dest.room), first, nbytes, t.fmt, t.P, idx) == m
            assert torch.equal(dest.got(m), src[first: first + m])
            plain_stats = ctx.last_decode_range_stats()
            assert checked_stats[0] <= plain_stats[0] and checked_stats[2] >= plain_stats[2], (t.name, first, nbytes)
        # the same reads in one call each way
        outs = [torch.full((max(0, min(nb, L - f)) + 8,), 0xA5, dtype=torch.uint8, device="cuda") for f, nb in rs]
        caps = [o.numel() - 8 for o in outs]
        firsts, nbs = [f for f, _ in rs], [nb for _, nb in rs]
        lens, status = ctx.decode_ranges_checked(s, len(t.s), firsts, nbs, outs, cks, L, caps, t.fmt, t.P, idx)
        assert status == [0] * len(rs) and lens == caps, t.name
        for o, (f, nb), m in zip(outs, rs, caps):
            assert torch.equal(o[:m], src[f: f + m]) and bool((o[m:] == 0xA5).all()), (t.name, f, nb)
        outs2 = [torch.empty_like(o) for o in outs]
        lens2, status2 = ctx.decode_ranges(s, len(t.s), firsts, nbs, outs2, caps, t.fmt, t.P, idx)
        assert (lens2, status2) == (lens, status)
        assert all(torch.equal(a[:m], b[:m]) for a, b, m in zip(outs, outs2, caps))


# ---- damage ---------------------------------------------------------------------------------------------------------------------

def damage_on_device(c):
    t = c.stream
    s, idx, cks, src = on_device(t)
    return (s if c.s is t.s else dev(c.s)), idx, (cks if c.cks is t.cks else dev_cks(c.cks)), src


def test_damage_single_read(ctx, oracle):
    cases = cc.damages(oracle)[0]
    dest = Dest(40000)
    seen = set()
    for c in cases:
        t = c.stream
        s, idx, cks, src = damage_on_device(c)
        L, w = len(t.data), len(t.s)
        hit, clean = cc.touching_range(c)
        seen.add(c.verdict)
        if c.verdict == "arg":
            p = dest.ptr()
            assert raw_checked(ctx, s, w, t.fmt, t.P, idx, cks, c.total_len, hit[0], hit[1], p, hit[1])[0] == zz.E_ARG, c.name
            assert dest.untouched_outside(0)
            continue
        if c.verdict == "call":                                 # the sidecar (or total_len) is not this stream's: every read is refused
            for first, nbytes in (hit, clean or hit, (0, L)):
                p = dest.ptr()
                assert raw_checked(ctx, s, w, t.fmt, t.P, idx, cks, c.total_len, first, nbytes, p, min(nbytes, dest.room)) == (zz.E_DATA, ERR), c.name
                assert dest.untouched_outside(0), c.name
                assert b"fold" in zz.lib.zz_last_error()
            continue
        # a damaged packet: the checked read refuses it, whole or in part ...
        for first, nbytes in (hit, (hit[0] + min(3, hit[1] - 1), 1), (max(0, hit[0] - 5), 10)):
            p = dest.ptr()
            assert raw_checked(ctx, s, w, t.fmt, t.P, idx, cks, L, first, nbytes, p, nbytes) == (zz.E_DATA, ERR), (c.name, first, nbytes)
            assert dest.untouched_outside(nbytes), c.name
        assert b"checksum mismatch" in zz.lib.zz_last_error()
        # ... where the unchecked read says ZZ_OK and hands back a wrong byte
        p = dest.ptr()
        assert ctx.decode_range(s, w, p, hit[1], hit[0], hit[1], t.fmt, t.P, idx) == hit[1], c.name
        wrong = cc.zlib_bytes(t, c.s)[hit[0]: hit[0] + hit[1]]
        assert bytes(dest.got(hit[1]).cpu().tolist()) == wrong != t.data[hit[0]: hit[0] + hit[1]], c.name
        # a read that does not touch the damaged packet is served
        if clean:
            p = dest.ptr()
            m = ctx.decode_range_checked(s, w, p, clean[1], clean[0], clean[1], cks, L, t.fmt, t.P, idx)
            assert m == min(clean[1], L - clean[0]) and torch.equal(dest.got(m), src[clean[0]: clean[0] + m]), c.name
            assert dest.untouched_outside(m)
    assert seen == {"packet", "call", "arg"}


def test_damage_multi_read(ctx, oracle):
    for c in cc.damages(oracle)[0]:
        t = c.stream
        if c.verdict == "arg":
            continue
        s, idx, cks, src = damage_on_device(c)
        L, w, P = len(t.data), len(t.s), t.P
        hit, clean = cc.touching_range(c)
        rs = [hit, clean or hit, (hit[0] + 1, 2), (0, min(L, 3 * P)), clean or hit, (max(0, hit[0] - 1), 2)]
        caps = [min(nb, L - f) for f, nb in rs]
        caps[3] -= 1                                            # this one does not fit
        outs = [torch.full((min(nb, L - f) + 8,), 0xA5, dtype=torch.uint8, device="cuda") for f, nb in rs]
        if c.verdict == "call":
            with pytest.raises(zz.ZzFlateError) as e:
                ctx.decode_ranges_checked(s, w, [f for f, _ in rs], [nb for _, nb in rs], outs, cks, c.total_len, caps, t.fmt, P, idx)
            assert e.value.code == zz.E_DATA and all(bool((o == 0xA5).all()) for o in outs), c.name
            continue
        lens, status = ctx.decode_ranges_checked(s, w, [f for f, _ in rs], [nb for _, nb in rs], outs, cks, L, caps, t.fmt, P, idx)
        for r, ((f, nb), o) in enumerate(zip(rs, outs)):
            k0, k1 = f // P, (f + nb - 1) // P + 1
            touched = any(k0 <= k < k1 for k in c.bad)
            want = zz.E_DATA if touched else zz.E_NOSPACE if r == 3 else 0
            assert status[r] == want, (c.name, r, status)
            if want == 0:
                assert lens[r] == caps[r] and torch.equal(o[: caps[r]], src[f: f + caps[r]]), (c.name, r)
            else:
                assert lens[r] is None and bool((o == 0xA5).all()), (c.name, r)                # a failed read is not copied
            assert bool((o[caps[r]:] == 0xA5).all())
        assert status.count(zz.E_DATA) >= 3 and (clean is None or status.count(0) >= 2), (c.name, status)


# ---- long ranges ----------------------------------------------------------------------------------------------------------------

def test_damage_in_the_second_batch_of_a_long_range(ctx):
    n, P = 80 << 20, 32768
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 3, 0, src, n)
    cap = zz.bound(n, 0, 0, P) + 64
    stream = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, n, stream, cap, 0, 0, P)
    idx = ctx.packet_index()
    cks = ctx.packet_checksums(src, n, 0, P)
    first, nbytes = (5 << 20) + 12345, 70 << 20
    buf = torch.full((nbytes + 2 * GUARD + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ctx.decode_range_checked(stream, w, buf.data_ptr() + GUARD + 1, nbytes, first, nbytes, cks, n, 0, P, idx) == nbytes
    assert torch.equal(buf[GUARD + 1: GUARD + 1 + nbytes], src[first: first + nbytes])
    assert bool((buf[: GUARD + 1] == 0xA5).all()) and bool((buf[GUARD + 1 + nbytes:] == 0xA5).all())
    fp, npk, tries, _ = ctx.last_decode_range_stats()
    assert npk * P > (64 << 20)                                 # more than one batch
    k = fp + (64 << 20) // P + 50                               # a packet of the second batch: one stored byte changed
    at = 2 + int(idx[k].item()) + 5 + 100
    stream[at] ^= 0x40
    rc, out = raw_checked(ctx, stream, w, 0, P, idx, cks, n, first, nbytes, buf.data_ptr() + GUARD + 1, nbytes)
    assert (rc, out) == (zz.E_DATA, ERR)
    assert bool((buf[: GUARD + 1] == 0xA5).all()) and bool((buf[GUARD + 1 + nbytes:] == 0xA5).all())
    assert ctx.decode_range(stream, w, buf.data_ptr() + GUARD + 1, nbytes, first, nbytes, 0, P, idx) == nbytes     # the unchecked read: served
    assert not torch.equal(buf[GUARD + 1: GUARD + 1 + nbytes], src[first: first + nbytes])
    # a range that ends in front of the damaged packet is served
    short = (k - first // P - 1) * P
    assert ctx.decode_range_checked(stream, w, buf.data_ptr() + GUARD + 1, short, first, short, cks, n, 0, P, idx) == short
    assert torch.equal(buf[GUARD + 1: GUARD + 1 + short], src[first: first + short])
    del buf, src, stream
    torch.cuda.empty_cache()


def test_look_back_that_grows(oracle):
    """P = 1000 at level 3 with a warm window: matches reach up to 32 KiB back, the first look-back of one packet is not enough"""
    c = zz.Context(0)
    c.set_warm_window(32768)
    data = cc.corpus_file("alice29.txt")[:150001]
    src = dev(data)
    L, P = len(data), 1000
    cap = zz.bound(L, 0, 3, P) + 64
    stream = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = c.encode(src, L, stream, cap, 0, 3, P)
    idx = c.packet_index()
    cks = c.packet_checksums(src, L, 0, P)
    assert patterns(cks) == zz.packet_checksums_host(data, 0, P)
    a = torch.empty(L, dtype=torch.uint8, device="cuda")
    b = torch.empty(L, dtype=torch.uint8, device="cuda")
    grew = 0
    for first, nbytes in ranges_for(L, P, 3)[:40]:
        m = c.decode_range_checked(stream, w, a, min(nbytes, L), first, nbytes, cks, L, 0, P, idx)
        tries = c.last_decode_range_stats()[2]
        assert c.decode_range(stream, w, b, min(nbytes, L), first, nbytes, 0, P, idx) == m == max(0, min(nbytes, L - first))
        assert torch.equal(a[:m], b[:m]) and torch.equal(a[:m], src[first: first + m]), (first, nbytes)
        assert tries >= c.last_decode_range_stats()[2]
        grew += tries > 1
    assert grew > 0
    rs = ranges_for(L, P, 4)[:40]
    outs = [torch.empty(max(0, min(nb, L - f)) + 1, dtype=torch.uint8, device="cuda") for f, nb in rs]
    lens, status = c.decode_ranges_checked(stream, w, [f for f, _ in rs], [nb for _, nb in rs], outs, cks, L, None, 0, P, idx)
    assert status == [0] * len(rs) and c.last_decode_ranges_stats()[2] > 0          # some reads came back with a longer look-back
    assert all(torch.equal(o[:m], src[f: f + m]) for o, (f, _), m in zip(outs, rs, lens))
    c.close()


# ---- state ----------------------------------------------------------------------------------------------------------------------

def test_state_is_left_as_the_unchecked_calls_leave_it(ctx, oracle):
    t = cc.stream(oracle, "alice29.txt_l2_P4096")
    s, idx, cks, src = on_device(t)
    L, w, P = len(t.data), len(t.s), t.P
    cap = zz.bound(L, 1, 2, P) + 64
    mine = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    mw = ctx.encode(src, L, mine, cap, 1, 2, P)
    out = torch.empty(L, dtype=torch.uint8, device="cuda")
    assert ctx.decode(mine, mw, out, L, 1, P, None) == L

    def state():
        return (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_index().cpu().tolist(), ctx.packet_index().cpu().tolist(),
                ctx.verify_last())
    before = state()
    assert ctx.decode_range(s, w, out, 9000, 50000, 9000, t.fmt, P, idx) == 9000
    plain = ctx.last_decode_range_stats()
    assert ctx.decode_range_checked(s, w, out, 100, 7, 100, cks, L, t.fmt, P, idx) == 100
    assert ctx.last_decode_range_stats()[:3] == (0, 1, 1)
    assert ctx.decode_range_checked(s, w, out, 9000, 50000, 9000, cks, L, t.fmt, P, idx) == 9000
    assert ctx.last_decode_range_stats() == plain                                   # the same packets, attempts and pending bytes
    bad = cks.clone(); bad[3] ^= 1
    with pytest.raises(zz.ZzFlateError):
        ctx.decode_range_checked(s, w, out, 100, 7, 100, bad, L, t.fmt, P, idx)
    assert ctx.last_decode_range_stats() == plain                                   # a failed read leaves the last successful one's
    ctx.decode_ranges(s, w, [5, 20000], [10, 5000], [out[:10], out[10:5010]], None, t.fmt, P, idx)
    multi = ctx.last_decode_ranges_stats()
    ctx.decode_ranges_checked(s, w, [7], [3], [out[:3]], cks, L, None, t.fmt, P, idx)
    assert ctx.last_decode_ranges_stats() != multi
    ctx.decode_ranges_checked(s, w, [5, 20000], [10, 5000], [out[:10], out[10:5010]], cks, L, None, t.fmt, P, idx)
    assert ctx.last_decode_ranges_stats() == multi and ctx.last_decode_range_stats() == plain
    ctx.packet_checksums(src, L, t.fmt, P)
    assert state() == before
    with pytest.raises(TypeError):
        ctx.decode_range_checked(s, w, out, 100, 7, 100, cks, None, t.fmt, P, idx)
    with pytest.raises(ValueError):
        ctx.decode_range_checked(s, w, out, 100, 7, 100, cks[:-1], L, t.fmt, P, idx)
    with pytest.raises(ValueError):
        ctx.decode_range_checked(s, w, out, 100, 7, 100, cks.cpu(), L, t.fmt, P, idx)
