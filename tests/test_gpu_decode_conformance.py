"""The device decoder's verdict against zlib's: the streams of tests/deflate_cases.py -- hand-made boundary streams, damaged zlib
streams, packet-mode streams written by zlib; every one has passed the bounds-checked CPU run of test_inflate_conformance_cpu.py,
which shares generator and seeds -- through zz_decode_batch_device (one call per list, raw DEFLATE, every staging alignment), the
serial path of zz_decode_device (raw, zlib and gzip containers), and its indexed and discovered paths, zz_decode_range_device and
zz_decode_ranges_device on the foreign packet streams. A stream zlib decodes gives exactly zlib's bytes, one zlib refuses gives
E_DATA, one that outgrows the destination E_DATA or E_NOSPACE, and nothing is written outside a destination. Needs a real
MI355X: run with `-m gpu`."""
import zlib

import pytest

import zzflate_amd as zz
from deflate_cases import (CAP, FOREIGN_FAMILIES, boundary_cases, corpus, expects_chains, expects_pending, foreign_streams,
                           front_of_stream, mutations, verdict, verdict_counts)
from range_streams import ranges_for

pytestmark = pytest.mark.gpu
GUARD = 32
N_MUTATIONS, SEED = 20000, 1          # as test_inflate_conformance_cpu.py
N_SERIAL = 300


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


def dev(torch, b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


class Blob:
    """all sources in one allocation, 0xFF between them: item i starts at an address congruent to i % 64 modulo 64, so every
    alignment of the decoder's 64-byte aligned staging occurs, and a byte read past an item's end is not a zero"""

    def __init__(self, torch, streams):
        self.offs, at = [], 64
        for i, s in enumerate(streams):
            at = (at + 63) // 64 * 64 + i % 64
            self.offs.append(at)
            at += len(s)
        host = bytearray(b"\xFF" * (at + 192))
        for o, s in zip(self.offs, streams):
            host[o: o + len(s)] = s
        self.t = torch.frombuffer(host, dtype=torch.uint8).cuda()
        assert self.t.data_ptr() % 64 == 0                   # (the allocator aligns far more coarsely)
        self.lens = [len(s) for s in streams]

    def items(self):
        p = self.t.data_ptr()
        assert all((p + o) % 64 == i % 64 for i, o in enumerate(self.offs))
        return [(p + o, n) for o, n in zip(self.offs, self.lens)]


class Slots:
    """one buffer of 0xEE cut into destinations, a guard between any two. The destinations with exact[i] set (the items expected
    to decode: their capacity is their length) lie in a first region, at an odd address for odd i and a 16-byte aligned one for
    even i, and come back to the host; the others (a failed item's destination is unspecified) lie behind them at a stride of
    cap + GUARD + 1, and only their guards are looked at, on the device."""

    def __init__(self, torch, caps, exact):
        self.torch, self.caps, self.exact = torch, list(caps), list(exact)
        self.offs, at = [0] * len(caps), 256
        for i, c in enumerate(caps):
            if exact[i]:
                at = (at + GUARD + 15) // 16 * 16 + (i & 1)
                self.offs[i] = at
                at += c
        self.a_end = at + GUARD
        self.rest = [i for i in range(len(caps)) if not exact[i]]
        self.slot = max([caps[i] for i in self.rest], default=0) + GUARD + 1
        for j, i in enumerate(self.rest):
            self.offs[i] = self.a_end + j * self.slot + GUARD + 1
        total = self.a_end + len(self.rest) * self.slot + GUARD + 256
        self.buf = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    def items(self):
        p = self.buf.data_ptr()
        return [(p + o, c) for o, c in zip(self.offs, self.caps)]

    def check(self, want):
        """destination i with exact[i] holds want[i] (bytes of its capacity or fewer: the rest is untouched), and nothing outside
        any destination was written"""
        host = self.buf[: self.a_end].cpu().numpy().tobytes()
        exp = bytearray(b"\xEE" * self.a_end)
        for i, w in enumerate(want):
            if self.exact[i]:
                exp[self.offs[i]: self.offs[i] + len(w)] = w
        if host != bytes(exp):
            for i, w in enumerate(want):
                if self.exact[i]:
                    o = self.offs[i]
                    assert host[o - GUARD: o + self.caps[i] + GUARD] == bytes(exp[o - GUARD: o + self.caps[i] + GUARD]), ("destination", i)
            raise AssertionError("bytes outside every destination were written")
        if self.rest:
            body = self.buf[self.a_end: self.a_end + len(self.rest) * self.slot].view(len(self.rest), self.slot)
            assert bool((body[:, : GUARD + 1] == 0xEE).all()), "a guard in front of a failed item's destination was written"
            for j, i in enumerate(self.rest):
                if self.caps[i] + GUARD + 1 < self.slot:
                    assert bool((body[j, GUARD + 1 + self.caps[i]:] == 0xEE).all())
        assert bool((self.buf[self.a_end + len(self.rest) * self.slot:] == 0xEE).all())


def batch(torch, ctx, srcs, dsts):
    """zz_decode_batch_device on raw DEFLATE items: (return value, lengths, status)"""
    k = len(srcs)
    table = torch.tensor([[p for p, _ in srcs], [n for _, n in srcs], [p for p, _ in dsts], [c for _, c in dsts]],
                         dtype=torch.int64).cuda()
    lens = torch.full((k,), 7, dtype=torch.int64, device="cuda")
    status = torch.full((k,), 7, dtype=torch.int32, device="cuda")
    rc = zz.lib.zz_decode_batch_device(ctx._h, k, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(),
                                       lens.data_ptr(), status.data_ptr(), 2, None)
    torch.cuda.synchronize()
    return rc, lens.cpu().tolist(), status.cpu().tolist()


def precedence(status):
    """the documented return value of a batch with these statuses"""
    if any(s in (zz.E_DATA, zz.E_UNSUPPORTED) for s in status):
        return zz.E_DATA
    return zz.E_NOSPACE if zz.E_NOSPACE in status else 0


def check_batch(torch, ctx, cases):
    """cases: (raw stream, verdict, zlib's bytes or None), all in ONE call"""
    blob = Blob(torch, [c[0] for c in cases])
    caps = [len(c[2]) if c[1] == "ok" else CAP for c in cases]
    slots = Slots(torch, caps, [c[1] == "ok" for c in cases])
    rc, lens, status = batch(torch, ctx, blob.items(), slots.items())
    for i, (raw, v, data) in enumerate(cases):
        if v == "ok":
            assert (status[i], lens[i]) == (0, len(data)), (i, status[i], lens[i])
        elif v == "bad":
            assert (status[i], lens[i]) == (zz.E_DATA, -1), (i, status[i], lens[i])
        else:
            assert status[i] in (zz.E_DATA, zz.E_NOSPACE) and lens[i] == -1, (i, status[i], lens[i])
    slots.check([c[2] for c in cases])
    assert rc == precedence(status)
    return status


def test_batch_boundary_cases(torch, ctx):
    cases = [(raw, v, data) for _, raw, v, data in boundary_cases()]
    print("boundary cases per verdict:", verdict_counts(cases, 1))
    status = check_batch(torch, ctx, cases)
    assert zz.E_DATA in status
    # the return value without a data failure: every item good, then some one byte short
    good = [c for c in cases if c[1] == "ok" and c[2]]
    blob = Blob(torch, [c[0] for c in good])
    slots = Slots(torch, [len(c[2]) for c in good], [True] * len(good))
    rc, lens, status = batch(torch, ctx, blob.items(), slots.items())
    assert rc == 0 and status == [0] * len(good) and lens == [len(c[2]) for c in good]
    slots.check([c[2] for c in good])
    short = [i % 5 == 2 for i in range(len(good))]
    slots = Slots(torch, [len(c[2]) - s for c, s in zip(good, short)], [not s for s in short])
    rc, lens, status = batch(torch, ctx, blob.items(), slots.items())
    assert rc == zz.E_NOSPACE and status == [zz.E_NOSPACE if s else 0 for s in short]
    assert lens == [-1 if s else len(c[2]) for c, s in zip(good, short)]
    slots.check([c[2] for c in good])


def test_batch_mutations(torch, ctx):
    cases = mutations(N_MUTATIONS, SEED)
    print("mutations per verdict:", verdict_counts(cases, 1))
    check_batch(torch, ctx, cases)


def test_batch_staging_edges(torch, ctx):
    """one stream at each of the 64 alignments, its source cut to every length around the first and the second restage of the
    2 KiB input stage: the cut streams are not streams, the whole one is"""
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    data = corpus("alice29.txt")[:16000]
    raw = co.compress(data) + co.flush()
    assert 5000 < len(raw) < 8000
    cuts = list(range(2030, 2061)) + list(range(4080, 4111)) + [len(raw)]
    cases = []
    for cut in cuts:
        v, d = verdict(raw[:cut], CAP)
        assert v == ("ok" if cut == len(raw) else "bad") and d == (data if cut == len(raw) else None)
        cases += [(raw[:cut], v, d)] * 64                    # (item i lies at alignment i % 64)
    check_batch(torch, ctx, cases)


def serial(torch, ctx, cases):
    """Context.decode(packet_size=0): raw, and what decodes again inside a zlib and a gzip container"""
    calls = []                                               # (stream, format, verdict, bytes)
    for raw, v, data in cases:
        calls.append((raw, 2, v, data))
        if v == "ok":
            calls.append((b"\x78\x01" + raw + zlib.adler32(data).to_bytes(4, "big"), 0, v, data))
            calls.append((b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + zlib.crc32(data).to_bytes(4, "little")
                          + (len(data) & 0xFFFFFFFF).to_bytes(4, "little"), 1, v, data))
    blob = Blob(torch, [c[0] for c in calls])
    out = torch.empty(max(CAP, max(len(c[3]) for c in calls if c[3] is not None)) + GUARD, dtype=torch.uint8, device="cuda")
    for i, ((ptr, n), (s, fmt, v, data)) in enumerate(zip(blob.items(), calls)):
        cap = len(data) if v == "ok" else CAP
        out.fill_(0xEE)
        if v == "ok":
            assert ctx.decode(ptr, n, out, cap, fmt, 0) == len(data), (i, fmt)
            assert ctx.last_decode_path() == zz.DECODE_SERIAL
            assert out[: cap + GUARD].cpu().numpy().tobytes() == data + b"\xEE" * GUARD, (i, fmt)
        else:
            with pytest.raises(zz.ZzFlateError) as e:
                ctx.decode(ptr, n, out, cap, fmt, 0)
            assert e.value.code in ((zz.E_DATA,) if v == "bad" else (zz.E_DATA, zz.E_NOSPACE)), (i, e.value.code)
            assert bool((out[cap:] == 0xEE).all()), i


def test_serial_path_boundary_cases(torch, ctx):
    serial(torch, ctx, [(raw, v, data) for _, raw, v, data in boundary_cases()])


def test_serial_path_mutations(torch, ctx):
    serial(torch, ctx, mutations(N_MUTATIONS, SEED)[:N_SERIAL])


def stats_hold(ctx, family, P, strategy):
    pend, rounds = ctx.last_decode_stats()
    if expects_pending(family, strategy):
        assert pend > 0, "expected matches that reach in front of a packet's start"
    if expects_chains(family, P, strategy):
        assert rounds > 1, "expected chains of more than one link"


@pytest.mark.parametrize("family", FOREIGN_FAMILIES)
def test_foreign_packet_streams(torch, ctx, family):
    for P, strategy, s, idx, data in foreign_streams(family):
        what = (family, P, strategy)
        L = len(data)
        st, ix = dev(torch, s), torch.tensor(idx, dtype=torch.int64).cuda()
        want = data + b"\xEE" * GUARD
        # the whole stream: with its index, and with the index found on the device
        for index, path in ((ix, zz.DECODE_INDEXED), (None, zz.DECODE_DISCOVERED)):
            out = torch.full((L + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
            assert ctx.decode(st, len(s), out, L, 0, P, index) == L, what
            assert ctx.last_decode_path() == path, what
            assert out.cpu().numpy().tobytes() == want, what
            stats_hold(ctx, family, P, strategy)
        assert ctx.last_decode_index().cpu().tolist() == idx, what
        # ranges: one by one, and all in one call
        reads = ranges_for(L, P, P + strategy)
        one = torch.full((L + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        for f, nb in reads[:4] + reads[7:13]:
            m = ctx.decode_range(st, len(s), one, min(nb, L), f, nb, 0, P, ix)
            assert m == max(0, min(nb, L - f)) and one[:m].cpu().numpy().tobytes() == data[f: f + m], (what, f, nb)
        assert bool((one[L:] == 0xEE).all())
        caps = [min(nb, L) for _, nb in reads]
        slots = Slots(torch, caps, [True] * len(reads))
        lens, status = ctx.decode_ranges(st, len(s), [f for f, _ in reads], [nb for _, nb in reads], slots.items(), caps, 0, P, ix)
        assert status == [0] * len(reads), (what, status)
        assert lens == [max(0, min(nb, L - f)) for f, nb in reads], what
        slots.check([data[f: f + nb] for f, nb in reads])
        # a lying index: an error or the exact bytes
        for d in (-1, 1):
            lie = list(idx); lie[len(idx) // 2] += d
            out = torch.full((L + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
            try:
                n = ctx.decode(st, len(s), out, L, 0, P, torch.tensor(lie, dtype=torch.int64).cuda())
            except zz.ZzFlateError as e:
                assert e.code == zz.E_DATA, (what, e.code)
            else:
                assert n == L and out.cpu().numpy().tobytes() == want, what


def test_first_match_in_front_of_the_stream(torch, ctx):
    P = 1000
    s, idx = front_of_stream(P)
    st, ix = dev(torch, s), torch.tensor(idx, dtype=torch.int64).cuda()
    out = torch.full((4000 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    for index in (ix, None):
        with pytest.raises(zz.ZzFlateError) as e:
            ctx.decode(st, len(s), out, 4000, 0, P, index)
        assert e.value.code == zz.E_DATA
    with pytest.raises(zz.ZzFlateError) as e:
        ctx.decode_range(st, len(s), out, 500, 100, 500, 0, P, ix)
    assert e.value.code == zz.E_DATA
    slots = Slots(torch, [5, 10], [False, False])
    lens, status = ctx.decode_ranges(st, len(s), [0, 500], [5, 10], slots.items(), [5, 10], 0, P, ix)
    assert status == [zz.E_DATA] * 2 and lens == [None] * 2
    slots.check([None, None])
    assert bool((out[4000:] == 0xEE).all())
