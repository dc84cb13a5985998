"""Many reads of one stream in one call on the device (zz_decode_ranges_device): every list of ranges goes in as ONE call into one
guarded buffer cut into destinations at odd and at 16-byte aligned addresses; every read equals the input's slice, has the
documented length, leaves its guards alone and is byte-equal to what decode_range returns for it alone. The hand-made streams
with known pointer chains, every status in one call, more than one wave, locality, and the context's state."""
import os
import random

import pytest

from conftest import CORPUS
from range_streams import HAND_P, hand_stream, ranges_for

torch = pytest.importorskip("torch")
import zzflate_amd as zz  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 32


@pytest.fixture(scope="module")
def ctx():
    c = zz.Context(0)
    yield c
    c.close()


def dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def encode(c, src, n, fmt, lvl, P):
    cap = zz.bound(n, fmt, min(lvl, 3), P) + 64
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = c.encode(src, n, dst, cap, fmt, lvl, P)
    return dst[:w].clone(), w, c.packet_index()


class Dests:
    """one buffer of 0xA5 cut into destinations of the given capacities, a guard between any two; destination i lies at an odd
    address for odd i and at a 16-byte aligned one for even i"""

    def __init__(self, caps):
        base_align = 256
        self.offs, at = [], base_align
        for i, c in enumerate(caps):
            at = (at + GUARD + 15) // 16 * 16 + (i & 1)
            self.offs.append(at)
            at += c
        self.buf = torch.full((at + GUARD + base_align,), 0xA5, dtype=torch.uint8, device="cuda")
        self.shift = (-self.buf.data_ptr()) % 16
        self.caps = list(caps)
        self.offs = [o + self.shift for o in self.offs]

    def items(self):
        p = self.buf.data_ptr()
        assert all((p + o) % 16 == (i & 1) for i, o in enumerate(self.offs))
        return [(p + o, c) for o, c in zip(self.offs, self.caps)]

    def got(self, host, i, n):
        return host[self.offs[i]: self.offs[i] + n]

    def check(self, lens, want):
        """every read's bytes are `want[i]` (None: a failed read, whose destination is unspecified) and nothing else was written"""
        host = self.buf.cpu().numpy().tobytes()
        at = 0
        for i, (o, c) in enumerate(zip(self.offs, self.caps)):
            assert host[at: o] == b"\xA5" * (o - at), ("guard in front of read", i)
            if want[i] is None:
                at = o + c
            else:
                assert lens[i] == len(want[i]) and host[o: o + lens[i]] == want[i], ("read", i)
                at = o + lens[i]
        assert host[at:] == b"\xA5" * (len(host) - at)
        return host


def read_all(c, stream, w, fmt, P, idx, reads, L, caps=None):
    caps = [min(nb, L) for _, nb in reads] if caps is None else caps
    d = Dests(caps)
    lens, status = c.decode_ranges(stream, w, [f for f, _ in reads], [nb for _, nb in reads], d.items(), caps, fmt, P, idx)
    return d, lens, status


def check_ranges(c, stream, w, fmt, P, idx, data, seed, alone=True):
    L = len(data)
    reads = ranges_for(L, P, seed)
    d, lens, status = read_all(c, stream, w, fmt, P, idx, reads, L)
    assert status == [0] * len(reads), (P, fmt, status)
    assert lens == [max(0, min(nb, L - f)) for f, nb in reads]
    host = d.check(lens, [data[f: f + nb] for f, nb in reads])
    if alone:
        one = torch.empty(L, dtype=torch.uint8, device="cuda")
        for i, (f, nb) in enumerate(reads):
            m = c.decode_range(stream, w, one, min(nb, L), f, nb, fmt, P, idx)
            assert m == lens[i] and one[:m].cpu().numpy().tobytes() == d.got(host, i, m), (P, fmt, f, nb)


@pytest.fixture(scope="module")
def files():
    out = {}
    for name in ("alice29.txt", "kennedy.xls"):
        data = open(os.path.join(CORPUS, name), "rb").read()[:300001]
        out[name] = (data, dev(data))
    return out


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_ranges_of_corpus_streams(ctx, files, lvl, fmt):
    for name, (data, src) in files.items():
        for P in (32768, 4096, 1000):
            stream, w, idx = encode(ctx, src, len(data), fmt, lvl, P)
            check_ranges(ctx, stream, w, fmt, P, idx, data, lvl * 3 + fmt)


@pytest.mark.parametrize("lvl,warm", [(2, 32768), (6, 0)])
def test_ranges_of_streams_that_reach_far_back(files, lvl, warm):
    c = zz.Context(0)
    c.set_extended_levels(True)
    c.set_warm_window(warm)
    data, src = files["alice29.txt"]
    for P in (32768, 4096, 1000):
        stream, w, idx = encode(c, src, len(data), 0, lvl, P)
        check_ranges(c, stream, w, 0, P, idx, data, lvl)
    c.close()


def test_hand_made_streams(ctx):
    P = HAND_P
    reads = [(41 * P - 1, 1), (10, 300), (P + 5, 100), (40 * P + 100, 300), (30 * P - 1, 1), (0, P)]
    for kind in ("a", "b"):
        s, idx, d = hand_stream(kind)
        st, ix = dev(s), torch.tensor(idx, dtype=torch.int64).cuda()
        dst, lens, status = read_all(ctx, st, len(s), 0, P, ix, reads, len(d))
        assert status == [0] * len(reads)
        dst.check(lens, [d[f: f + nb] for f, nb in reads])
        packets, attempts, retried, waves = ctx.last_decode_ranges_stats()
        assert attempts >= 2 and retried >= 1 and waves >= attempts
        if kind == "a":
            # the first attempt: 2 + 1 + 2 + 2 + 2 + 1 packets; then the one read with look-backs 4, 16, 40
            assert retried == 1 and attempts == 4 and packets == 10 + 5 + 17 + 41
        check_ranges(ctx, st, len(s), 0, P, ix, d, 5 if kind == "a" else 6)

    s, idx, d = hand_stream("c", 44)
    st, ix = dev(s), torch.tensor(idx, dtype=torch.int64).cuda()
    reads = [(0, 5), (500, 10), (P + 500, 10), (40 * P + 100, 300), (41 * P - 1, 1)]
    dst, lens, status = read_all(ctx, st, len(s), 0, P, ix, reads, 44 * P)
    assert status == [zz.E_DATA] * 4 + [0] and lens == [None] * 4 + [1]
    assert zz.lib.zz_last_error().startswith(b"reads: 4 ")
    dst.check(lens, [None] * 4 + [bytes([dst.buf[dst.offs[4]].item()])])


@pytest.fixture(scope="module")
def big():
    """80 MiB of generated text at level 2, 32 KiB packets, and its decoded bytes"""
    c = zz.Context(0)
    n = 80 << 20
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.generate(zz.GEN_TEXT, 3, 0, src, n)
    stream, w, idx = encode(c, src, n, 0, 2, 32768)
    c.close()
    yield n, src, stream, w, idx
    del src, stream
    torch.cuda.empty_cache()


def test_every_status_in_one_call(ctx, big):
    n, src, stream, w, idx = big
    P = 32768
    index = idx.cpu().tolist()
    bad = stream.clone()
    kbad = 100
    bad[2 + index[kbad + 1] - 5] ^= 0xFF                            # LEN of packet 100's closing stored block: no longer NLEN's complement
    bad[2 + index[kbad + 1] - 4] ^= 0xFF
    npk = len(index) - 1
    reads = [(5 * P + 7, 5000), (npk * P, 1), (7 * P, 3000), (kbad * P + 10, 100), ((kbad + 1) * P + 10, 100), ((kbad + 2) * P + 10, 100),
             ((5 << 20) + 12345, 70 << 20), (n - 100, 1000), (3, 0), (99 * P - 50, 20)]
    caps = [5000, 10, 2999, 100, 100, 100, 16, 100, 0, 20]
    d = Dests(caps)
    tab = torch.tensor([[f for f, _ in reads], [nb for _, nb in reads], [p for p, _ in d.items()], caps], dtype=torch.int64).cuda()
    lens = torch.empty(len(reads), dtype=torch.int64, device="cuda")
    status = torch.empty(len(reads), dtype=torch.int32, device="cuda")

    def raw(k, st):
        return zz.lib.zz_decode_ranges_device(ctx._h, bad.data_ptr(), w, 0, P, idx.data_ptr(), idx.numel(), k, tab[0].data_ptr(),
                                              tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), lens.data_ptr(), st, ctx._stream())
    assert raw(len(reads), status.data_ptr()) == zz.E_DATA
    want_status = [0, zz.E_ARG, zz.E_NOSPACE, zz.E_DATA, zz.E_DATA, 0, zz.E_UNSUPPORTED, 0, 0, 0]
    assert status.cpu().tolist() == want_status
    host_src = src.cpu().numpy().tobytes()
    want = [host_src[f: f + nb] if sv == 0 else None for (f, nb), sv in zip(reads, want_status)]
    got_lens = [None if v == -1 else v for v in lens.cpu().tolist()]
    assert got_lens == [5000, None, None, None, None, 100, None, 100, 0, 20]
    host = d.buf.cpu().numpy().tobytes()
    for i, wv in enumerate(want):
        if wv is not None:
            assert d.got(host, i, len(wv)) == wv, i
    # the precedence of the return value, without a status array
    order = [3, 6, 1, 2, 0]                                         # a DATA, the UNSUPPORTED, the ARG, the NOSPACE, an OK read
    for cut, rc in ((0, zz.E_DATA), (1, zz.E_UNSUPPORTED), (2, zz.E_ARG), (3, zz.E_NOSPACE), (4, 0)):
        pick = order[cut:]
        tab2 = tab[:, pick].contiguous()
        rc2 = zz.lib.zz_decode_ranges_device(ctx._h, bad.data_ptr(), w, 0, P, idx.data_ptr(), idx.numel(), len(pick), tab2[0].data_ptr(),
                                             tab2[1].data_ptr(), tab2[2].data_ptr(), tab2[3].data_ptr(), lens.data_ptr(), None, ctx._stream())
        assert rc2 == rc, (cut, rc2)
    # Python: a read's own failure does not raise
    lens2, status2 = ctx.decode_ranges(bad, w, [f for f, _ in reads], [nb for _, nb in reads], d.items(), caps, 0, P, idx)
    assert status2 == want_status and lens2 == got_lens


def test_more_than_one_wave(big):
    n, src, stream, w, idx = big
    P = 32768
    c = zz.Context(0)
    rng = random.Random(12)
    reads = [(rng.randrange(n - 300), rng.randrange(1, 301)) for _ in range(5000)]
    caps = [nb for _, nb in reads]
    d = Dests(caps)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    lens, status = c.decode_ranges(stream, w, [f for f, _ in reads], caps, d.items(), caps, 0, P, idx)
    free2 = torch.cuda.mem_get_info()[0]
    assert status == [0] * 5000 and lens == caps
    host_src = src.cpu().numpy().tobytes()
    d.check(lens, [host_src[f: f + nb] for f, nb in reads])
    packets, attempts, retried, waves = c.last_decode_ranges_stats()
    assert waves >= 2 and packets >= 10000 and attempts >= 1
    # the documented bound: two batches of packets (per packet its bytes, 4 bytes of pointer per byte, the bitmap, 44 bytes),
    # 48 bytes per read and the tables the host reads; 8 MiB of slack for the allocator's granules
    batch = (64 << 20) // P
    bound = 2 * batch * (P + 4 * P + P // 8 + 44) + 48 * 5000 + (64 << 10) + (8 << 20)
    assert free1 - free2 <= bound, (free1 - free2, bound)
    c.close()


@pytest.mark.parametrize("lvl,P", [(1, 4096), (2, 32768), (3, 1000)])
def test_locality(ctx, files, lvl, P):
    """the call reads the packets of its reads' segments and nothing else of the stream's packets"""
    data, src = files["kennedy.xls"]
    n = len(data)
    stream, w, idx = encode(ctx, src, n, 0, lvl, P)
    index = idx.cpu().tolist()
    rng = random.Random(lvl)
    reads = [(rng.randrange(n), rng.randrange(1, 3 * P)) for _ in range(6)]
    d, lens, status = read_all(ctx, stream, w, 0, P, idx, reads, n)
    assert status == [0] * 6
    host = d.check(lens, [data[f: f + nb] for f, nb in reads])
    # the segment of each read, as decode_range reports it for the read alone
    keep = set()
    one = torch.empty(n, dtype=torch.uint8, device="cuda")
    for f, nb in reads:
        ctx.decode_range(stream, w, one, min(nb, n), f, nb, 0, P, idx)
        fp, npk, _, _ = ctx.last_decode_range_stats()
        keep.update(range(fp, fp + npk))
    damaged = stream.clone()
    for k in range(len(index) - 1):
        if k not in keep:
            damaged[2 + index[k]: 2 + index[k + 1]] = 0xFF
    d2, lens2, status2 = read_all(ctx, damaged, w, 0, P, idx, reads, n)
    assert status2 == status and lens2 == lens and d2.buf.cpu().numpy().tobytes() == host


def test_state_is_left_alone(ctx, files):
    data, src = files["alice29.txt"]
    n, P = len(data), 4096
    stream, w, idx = encode(ctx, src, n, 0, 2, P)
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.decode(stream, w, out, n, 0, P, None) == n
    assert ctx.decode_range(stream, w, out, 9000, 50000, 9000, 0, P, idx) == 9000

    def state():
        return (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_index().cpu().tolist(), ctx.packet_index().cpu().tolist(),
                ctx.last_decode_range_stats())
    before = state()
    assert before[0] == zz.DECODE_DISCOVERED
    reads = [(50000, 9000), (0, 1), (n, 5)]
    d, lens, status = read_all(ctx, stream, w, 0, P, idx, reads, n)
    assert status == [0, 0, 0] and lens == [9000, 1, 0]
    with pytest.raises(zz.ZzFlateError) as e:                       # not a gzip header: the call fails, and raises
        read_all(ctx, stream, w, 1, P, idx, reads, n)
    assert e.value.code == zz.E_DATA
    with pytest.raises(TypeError):
        ctx.decode_ranges(stream, w, [0], [1], d.items()[:1], None, 0, P, None)
    with pytest.raises(ValueError):
        ctx.decode_ranges(stream, w, [0], [1], d.items()[:1], None, 0, P, idx.cpu())
    assert state() == before
    # a failure of the call marks every read
    tab = torch.tensor([[0, 5], [1, 1], [d.items()[0][0], d.items()[1][0]], [1, 1]], dtype=torch.int64).cuda()
    lens_t = torch.zeros(2, dtype=torch.int64, device="cuda")
    st_t = torch.zeros(2, dtype=torch.int32, device="cuda")

    def raw(c):
        return zz.lib.zz_decode_ranges_device(c._h, stream.data_ptr(), w, 1, P, idx.data_ptr(), idx.numel(), 2, tab[0].data_ptr(),
                                              tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), lens_t.data_ptr(), st_t.data_ptr(),
                                              c._stream())
    assert raw(ctx) == zz.E_DATA and st_t.cpu().tolist() == [zz.E_DATA] * 2 and lens_t.cpu().tolist() == [-1, -1]
    # an encode that has been enqueued but not finished: refused, and fine again after finish()
    cap = zz.bound(n, 0, 1, P)
    enc = torch.empty(cap, dtype=torch.uint8, device="cuda")
    c2 = zz.Context(0)
    c2.encode_async(src, n, enc, cap, 0, 1, P)
    with pytest.raises(zz.ZzFlateError) as e:
        read_all(c2, stream, w, 0, P, idx, reads, n)
    assert e.value.code == zz.E_ARG
    c2.finish()
    d3, lens3, status3 = read_all(c2, stream, w, 0, P, idx, reads, n)
    assert status3 == [0, 0, 0] and lens3 == [9000, 1, 0]
    d3.check(lens3, [data[50000:59000], data[0:1], b""])
    c2.close()
