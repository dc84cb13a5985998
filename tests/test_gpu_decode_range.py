"""Range decode on the device (zz_decode_range_device): bytes [first, first + n) of streams from ctx.encode with
ctx.packet_index(), compared with slices of the input; destinations with guard bytes at odd and at aligned addresses; the
hand-made streams with known pointer chains; capacity, locality, damage, a range longer than a batch, and the context's state.

Damage: the call does not check the trailer's checksum (it covers bytes the call never decodes), so a flipped byte that leaves a
packet's structure intact -- another literal of the same code length, another stored byte -- cannot be noticed by any range
reader. "ZZ_E_DATA or the exact bytes" is therefore asserted where the format itself decides: the length words of a packet's
closing stored block (LEN and NLEN must be complements, RFC 1951 3.2.4), in every packet the call decodes. For flips anywhere
else in a decoded packet the test asserts what holds for every input: ZZ_OK or ZZ_E_DATA, the documented length, and not one byte
outside the destination."""
import os
import random

import pytest

from conftest import CORPUS
from range_streams import HAND_P, hand_stream, ranges_for

torch = pytest.importorskip("torch")
import zzflate_amd as zz  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = zz.Context(0)
    yield c
    c.close()


def dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def corpus_file(name):
    return open(os.path.join(CORPUS, name), "rb").read()


def encode(c, src, n, fmt, lvl, P):
    cap = zz.bound(n, fmt, min(lvl, 3), P) + 64
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = c.encode(src, n, dst, cap, fmt, lvl, P)
    return dst[:w].clone(), w, c.packet_index()


class Dest:
    """a destination of `room` bytes filled with 0xA5 between two guards, at an odd or at a 16-byte aligned address"""

    def __init__(self, room):
        self.buf = torch.empty(room + 2 * GUARD + 32, dtype=torch.uint8, device="cuda")
        self.room = room

    def at(self, odd):
        self.buf.fill_(0xA5)
        off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 16 + (1 if odd else 0)
        assert (self.buf.data_ptr() + off) % 16 == (1 if odd else 0)
        self.off = off
        return self.buf.data_ptr() + off

    def untouched_outside(self, n):
        return bool((self.buf[: self.off] == 0xA5).all()) and bool((self.buf[self.off + n:] == 0xA5).all())

    def got(self, n):
        return self.buf[self.off: self.off + n]


def read(c, stream, w, fmt, P, idx, first, nbytes, dest, odd, cap=None):
    cap = min(nbytes, dest.room) if cap is None else cap
    p = dest.at(odd)
    return c.decode_range(stream, w, p, cap, first, nbytes, fmt, P, idx)


def check_ranges(c, stream, w, fmt, P, idx, src, L, seed, dest):
    for i, (first, nbytes) in enumerate(ranges_for(L, P, seed)):
        for odd in ((False, True) if i < 8 else (bool(i & 1),)):
            m = read(c, stream, w, fmt, P, idx, first, nbytes, dest, odd)
            assert m == max(0, min(nbytes, L - first)), (P, fmt, first, nbytes)
            assert torch.equal(dest.got(m), src[first: first + m]), (P, fmt, first, nbytes, c.last_decode_range_stats())
            assert dest.untouched_outside(m), (P, fmt, first, nbytes)
            fp, npk, tries, _ = c.last_decode_range_stats()
            assert fp <= first // P < fp + npk and tries >= 1


@pytest.fixture(scope="module")
def files():
    out = {}
    for name in ("alice29.txt", "kennedy.xls"):
        data = corpus_file(name)[:300001]
        out[name] = (data, dev(data), Dest(len(data)))
    return out


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_ranges_of_corpus_streams(ctx, files, lvl, fmt):
    for name, (data, src, dest) in files.items():
        for P in (32768, 4096, 1000):
            stream, w, idx = encode(ctx, src, len(data), fmt, lvl, P)
            check_ranges(ctx, stream, w, fmt, P, idx, src, len(data), lvl * 3 + fmt, dest)


@pytest.mark.parametrize("lvl,warm", [(2, 32768), (6, 0)])
def test_ranges_of_streams_that_reach_far_back(files, lvl, warm):
    c = zz.Context(0)
    c.set_extended_levels(True)
    c.set_warm_window(warm)
    data, src, dest = files["alice29.txt"]
    for P in (32768, 4096, 1000):
        stream, w, idx = encode(c, src, len(data), 0, lvl, P)
        check_ranges(c, stream, w, 0, P, idx, src, len(data), lvl, dest)
    c.close()


def test_index_recovered_by_discovery(ctx, files):
    data, src, dest = files["alice29.txt"]
    n = len(data)
    for P in (32768, 1000):
        stream, w, idx = encode(ctx, src, n, 1, 2, P)
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert ctx.decode(stream, w, out, n, 1, P, None) == n and ctx.last_decode_path() == zz.DECODE_DISCOVERED
        found = ctx.last_decode_index()
        assert torch.equal(found, idx)
        check_ranges(ctx, stream, w, 1, P, found, src, n, 11, dest)


def test_hand_made_streams(ctx):
    dest = Dest(50000)
    s, idx, d = hand_stream("a")
    st, ix, src = dev(s), torch.tensor(idx, dtype=torch.int64).cuda(), dev(d)
    first = 40 * HAND_P + 100
    assert read(ctx, st, len(s), 0, HAND_P, ix, first, 300, dest, True) == 300
    assert torch.equal(dest.got(300), src[first: first + 300]) and dest.untouched_outside(300)
    fp, npk, tries, pend = ctx.last_decode_range_stats()
    assert fp == 0 and npk == 41 and tries >= 2 and pend == 40 * (HAND_P - 1)
    assert read(ctx, st, len(s), 0, HAND_P, ix, 41 * HAND_P - 1, 1, dest, False) == 1
    assert ctx.last_decode_range_stats()[:3] == (39, 2, 1)
    check_ranges(ctx, st, len(s), 0, HAND_P, ix, src, len(d), 5, dest)

    s, idx, d = hand_stream("b")
    st, ix, src = dev(s), torch.tensor(idx, dtype=torch.int64).cuda(), dev(d)
    assert read(ctx, st, len(s), 0, HAND_P, ix, first, 300, dest, True) == 300
    assert torch.equal(dest.got(300), src[first: first + 300]) and dest.untouched_outside(300)
    assert ctx.last_decode_range_stats()[0] <= 37
    check_ranges(ctx, st, len(s), 0, HAND_P, ix, src, len(d), 6, dest)

    s, idx, d = hand_stream("c", 3)
    st, ix = dev(s), torch.tensor(idx, dtype=torch.int64).cuda()
    for first, nbytes in ((0, 5), (500, 10), (999, 2), (1500, 10)):
        with pytest.raises(zz.ZzFlateError) as e:
            read(ctx, st, len(s), 0, HAND_P, ix, first, nbytes, dest, False)
        assert e.value.code == zz.E_DATA and dest.untouched_outside(0)


def raw_call(c, stream, w, fmt, P, idx, first, nbytes, p, cap):
    import ctypes
    out = ctypes.c_uint64(5)
    rc = zz.lib.zz_decode_range_device(c._h, stream.data_ptr(), w, fmt, P, idx.data_ptr(), idx.numel(), first, nbytes, p, cap,
                                       ctypes.byref(out), c._stream())
    return rc, out.value


def test_capacity_and_arguments(ctx, files):
    data, src, dest = files["alice29.txt"]
    n, P = len(data), 4096
    stream, w, idx = encode(ctx, src, n, 0, 2, P)
    for first, nbytes in ((100, 10000), (n - 50, 1000), (0, n)):
        m = min(nbytes, n - first)
        for odd in (False, True):
            p = dest.at(odd)
            assert raw_call(ctx, stream, w, 0, P, idx, first, nbytes, p, m - 1) == (zz.E_NOSPACE, (1 << 64) - 1)
            assert dest.untouched_outside(m - 1)
            assert "destination too small for the range (%d bytes)" % m in zz.lib.zz_last_error().decode()
            p = dest.at(odd)
            assert raw_call(ctx, stream, w, 0, P, idx, first, nbytes, p, m) == (0, m) and dest.untouched_outside(m)
    p = dest.at(False)
    npk = idx.numel() - 1
    assert raw_call(ctx, stream, w, 0, P, idx, npk * P, 1, p, 10)[0] == zz.E_ARG
    assert raw_call(ctx, stream, w, 0, P, idx, 5, 0, p, 10) == (0, 0)
    assert raw_call(ctx, stream, w, 0, P, idx, n, 7, p, 10) == (0, 0)                   # behind the end, inside the last packet's span
    assert raw_call(ctx, stream, w, 1, P, idx, 0, 1, p, 10)[0] == zz.E_DATA             # not a gzip header
    assert raw_call(ctx, stream, w, 0, P, idx[:-1], 0, 1, p, 10)[0] == zz.E_DATA        # the index's end is not the stream's
    fdict = dev(b"\x78\xbb" + bytes(20))
    assert raw_call(ctx, fdict, 22, 0, P, idx, 0, 1, p, 10)[0] == zz.E_UNSUPPORTED
    with pytest.raises(TypeError):
        ctx.decode_range(stream, w, p, 10, 0, 1, 0, P, None)
    with pytest.raises(ValueError):
        ctx.decode_range(stream, w, p, 10, 0, 1, 0, P, idx.cpu())
    # an encode that has been enqueued but not finished: refused, and fine again after finish()
    cap = zz.bound(n, 0, 1, P)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    c2 = zz.Context(0)
    c2.encode_async(src, n, out, cap, 0, 1, P)
    assert raw_call(c2, stream, w, 0, P, idx, 0, 1, p, 10)[0] == zz.E_ARG
    c2.finish()
    assert raw_call(c2, stream, w, 0, P, idx, 0, 1, p, 10) == (0, 1)
    c2.close()
    assert dest.untouched_outside(1)


@pytest.mark.parametrize("lvl,P", [(1, 4096), (2, 32768), (3, 1000)])
def test_locality(ctx, files, lvl, P):
    """the call reads the packets it reports and nothing else of the stream's packets"""
    data, src, dest = files["kennedy.xls"]
    n = len(data)
    stream, w, idx = encode(ctx, src, n, 0, lvl, P)
    index = idx.cpu().tolist()
    rng = random.Random(lvl)
    for _ in range(6):
        first = rng.randrange(n)
        nbytes = rng.randrange(1, 3 * P)
        m = read(ctx, stream, w, 0, P, idx, first, nbytes, dest, True)
        assert torch.equal(dest.got(m), src[first: first + m])
        fp, npk, _, _ = ctx.last_decode_range_stats()
        damaged = stream.clone()
        damaged[2: 2 + index[fp]] = 0xFF
        damaged[2 + index[fp + npk]: 2 + index[-1]] = 0xFF
        m2 = read(ctx, damaged, w, 0, P, idx, first, nbytes, dest, True)
        assert m2 == m and torch.equal(dest.got(m), src[first: first + m]) and dest.untouched_outside(m)
        assert ctx.last_decode_range_stats()[:2] == (fp, npk)


def test_flipped_bytes(ctx, files):
    data, src, dest = files["alice29.txt"]
    n, P = len(data), 4096
    stream, w, idx = encode(ctx, src, n, 0, 2, P)
    index = idx.cpu().tolist()
    first, nbytes = 10 * P + 77, 2 * P
    m = read(ctx, stream, w, 0, P, idx, first, nbytes, dest, True)
    assert m == nbytes
    fp, npk, _, _ = ctx.last_decode_range_stats()
    # LEN / NLEN of the closing stored block of every decoded packet: the five bytes in front of the next packet's start
    for k in range(fp, fp + npk):
        for back, bit in ((5, 1), (4, 0x80), (3, 4), (2, 0x10)):
            bad = stream.clone()
            bad[2 + index[k + 1] - back] ^= bit
            p = dest.at(True)
            rc, out = raw_call(ctx, bad, w, 0, P, idx, first, nbytes, p, nbytes)
            assert rc == zz.E_DATA or (rc == 0 and out == m and torch.equal(dest.got(m), src[first: first + m])), (k, back)
            assert rc == zz.E_DATA, (k, back)                       # (these four bytes cannot be flipped unnoticed)
            assert dest.untouched_outside(nbytes)
    rng = random.Random(8)
    for _ in range(60):
        at = rng.randrange(index[fp], index[fp + npk])
        bad = stream.clone()
        bad[2 + at] ^= 1 << rng.randrange(8)
        p = dest.at(bool(at & 1))
        rc, out = raw_call(ctx, bad, w, 0, P, idx, first, nbytes, p, nbytes)
        assert (rc == 0 and out == m) or (rc == zz.E_DATA and out == 0), (at, rc, out)
        assert dest.untouched_outside(nbytes)


def test_range_longer_than_a_batch(ctx):
    n = 80 << 20
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 3, 0, src, n)
    stream, w, idx = encode(ctx, src, n, 0, 2, 32768)
    full = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.decode(stream, w, full, n, 0, 32768, idx) == n
    first, nbytes = (5 << 20) + 12345, 70 << 20
    buf = torch.full((nbytes + 2 * GUARD + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ctx.decode_range(stream, w, buf.data_ptr() + GUARD + 1, nbytes, first, nbytes, 0, 32768, idx) == nbytes
    assert torch.equal(buf[GUARD + 1: GUARD + 1 + nbytes], full[first: first + nbytes])
    assert bool((buf[: GUARD + 1] == 0xA5).all()) and bool((buf[GUARD + 1 + nbytes:] == 0xA5).all())
    fp, npk, tries, _ = ctx.last_decode_range_stats()
    assert fp <= first // 32768 and (fp + npk) * 32768 >= first + nbytes and npk * 32768 > (64 << 20)
    # the tail, clipped at the stream's end
    assert ctx.decode_range(stream, w, buf.data_ptr() + GUARD, nbytes, n - 1000, nbytes, 0, 32768, idx) == 1000
    assert torch.equal(buf[GUARD: GUARD + 1000], full[n - 1000:])
    del buf, full, src, stream
    torch.cuda.empty_cache()


def test_last_decode_state_is_left_alone(ctx, files):
    data, src, dest = files["alice29.txt"]
    n, P = len(data), 4096
    stream, w, idx = encode(ctx, src, n, 0, 2, P)
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.decode(stream, w, out, n, 0, P, None) == n
    before = (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_index().cpu().tolist(), ctx.packet_index().cpu().tolist())
    assert before[0] == zz.DECODE_DISCOVERED
    assert read(ctx, stream, w, 0, P, idx, 50000, 9000, dest, True) == 9000
    with pytest.raises(zz.ZzFlateError):
        read(ctx, stream, w, 1, P, idx, 50000, 9000, dest, True)
    after = (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_index().cpu().tolist(), ctx.packet_index().cpu().tolist())
    assert after == before
