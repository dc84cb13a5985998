"""Inputs that expand (tests/expansion_cases.py; the guards that need no GPU are in tests/test_expansion_cases_cpu.py): packets
within a byte or two of their slot, the stored fallback and the five k around its threshold, through every encoder form. Each
form's stream equals oracle.encode_packets(d, fmt, lvl, P, warm) byte for byte (a shard's: the oracle's packets), stays inside
zz_bound, reports no slot overflow (which would surface as E_NOSPACE "internal: packet slot overflow") and verifies on the
device where the form keeps a last call; the streams go back through decode_batch, every eighth through Context.decode with the
call's packet index. The container format cycles with the case's index. Needs a real MI355X: run with `-m gpu`.

A test is one (family, mode): about 120 inputs, 1 MiB in all, the largest 3 * 32768 + 1 bytes."""
import pytest

import expansion_cases as ec
import members_write_cases as mw
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
DECODE_EVERY = 8
GAP = 64                               # bytes of 0xA5 between neighbouring destinations; they must stay


def mode_id(m):
    return f"level{m[0]}" + (f"-warm{m[1]}" if m[1] else "")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


_items = {}


def items_of(oracle, family, lvl=None):
    """[(label, data, packet size, container)]: the family's cases, or the tipping cells of `lvl` with their five k each"""
    key = (family, lvl if family == "tipping" else None)
    if key not in _items:
        if family == "tipping":
            rows = [((L, final, k), *ec.tip_stream(d, final)) for L, cl, final in ec.tip_cells() if cl == lvl
                    for k, d in ec.tipping(oracle, L, cl, final)]
        else:
            rows = [(c, ec.data(c), c[2]) for c in ec.cases(family)]
        _items[key] = [(label, d, P, ec.fmt_of(i)) for i, (label, d, P) in enumerate(rows)]
    return _items[key]


def families(modes):
    """(family, mode) for the parametrisation: the tipping cells exist at levels 2 and above"""
    return [(f, m) for m in modes for f in ec.FAMILIES + ["tipping"] if f != "tipping" or m[0] >= 2]


def fm_id(p):
    return f"{p[0]}-{mode_id(p[1])}"


class Streams:
    """the inputs of a list of items back to back in one device buffer; destinations of caps[i] bytes each in another, filled
    with 0xA5 and GAP bytes apart"""

    def __init__(self, torch, items, caps):
        self.torch, self.items, self.caps = torch, items, caps
        self.soff, self.doff, at, to = [], [], 0, GAP
        for (_, d, _, _), cap in zip(items, caps):
            self.soff.append(at)
            self.doff.append(to)
            at += len(d)
            to += cap + GAP
        self.src = torch.frombuffer(bytearray(b"".join(d for _, d, _, _ in items)) or bytearray(1), dtype=torch.uint8).cuda()
        self.dst = torch.full((to,), 0xA5, dtype=torch.uint8, device="cuda")
        self.lens = [0] * len(items)

    def source(self, i):
        return self.src.data_ptr() + self.soff[i]

    def dest(self, i):
        return self.dst.data_ptr() + self.doff[i]

    def collect(self):
        """([stream], the items whose surroundings were written to)"""
        host = self.dst.cpu().numpy().tobytes()
        touched = [self.items[i][0] for i in range(len(self.items))
                   if host[self.doff[i] - GAP:self.doff[i]] != b"\xA5" * GAP or
                   host[self.doff[i] + self.caps[i]:self.doff[i] + self.caps[i] + GAP] != b"\xA5" * GAP]
        return [host[o:o + w] for o, w in zip(self.doff, self.lens)], touched

    def decode_batch(self, ctx):
        """every stream through Context.decode_batch, one call per container: the items that did not come back"""
        torch, bad = self.torch, []
        ooff, at = [], 0
        for _, d, _, _ in self.items:
            ooff.append(at)
            at += len(d) + 1
        out = torch.full((at,), 0xEE, dtype=torch.uint8, device="cuda")
        for fmt in range(3):
            ids = [i for i, it in enumerate(self.items) if it[3] == fmt]
            if not ids:
                continue
            lens, status = ctx.decode_batch([(self.dest(i), self.lens[i]) for i in ids],
                                            [(out.data_ptr() + ooff[i], len(self.items[i][1]) + 1) for i in ids], fmt)
            bad += [(self.items[i][0], "decode_batch", s, w) for i, s, w in zip(ids, status, lens) if s != 0 or w != len(self.items[i][1])]
        host = out.cpu().numpy().tobytes()
        for i, (label, d, _, _) in enumerate(self.items):
            if host[ooff[i]:ooff[i] + len(d) + 1] != d + b"\xEE":
                bad.append((label, "decode_batch bytes"))
        return bad


def single_calls(torch, ctx, oracle, items, lvl, warm, before_each=None):
    """Context.encode per item into a destination of zz_bound bytes, against the oracle"""
    caps = [zz.bound(len(d), fmt, lvl, P) for _, d, P, fmt in items]
    s = Streams(torch, items, caps)
    bad = []
    one = torch.zeros(ec.MAX_N + 2, dtype=torch.uint8, device="cuda")
    ctx.set_extended_levels(lvl > 3)
    ctx.set_warm_window(warm)
    try:
        for i, (label, d, P, fmt) in enumerate(items):
            if before_each:
                before_each()
            try:
                s.lens[i] = ctx.encode(s.source(i), len(d), s.dest(i), caps[i], fmt, lvl, P)
            except zz.ZzFlateError as e:
                bad.append((label, "encode raised", str(e)))
                continue
            if ctx.verify_last() != (0, None):
                bad.append((label, "verify_last"))
            if i % DECODE_EVERY == 0:
                w = ctx.decode(s.dest(i), s.lens[i], one, len(d) + 1, fmt, P, ctx.packet_index())
                if w != len(d) or one[:w].cpu().numpy().tobytes() != d:
                    bad.append((label, "decode"))
    finally:
        ctx.set_warm_window(0)
        ctx.set_extended_levels(False)
    streams, touched = s.collect()
    bad += [(t, "wrote outside its destination") for t in touched]
    for (label, d, P, fmt), got, cap in zip(items, streams, caps):
        if got != oracle.encode_packets(d, fmt, lvl, P, warm):
            bad.append((label, "encode", fmt, len(got)))
        if len(got) > cap:
            bad.append((label, "bound", len(got), cap))
    bad += s.decode_batch(ctx)
    assert bad == [], (lvl, warm, len(bad), bad[:8])


@pytest.mark.parametrize("fm", families(ec.COLD + ec.WARM), ids=fm_id)
def test_single_calls(torch, ctx, oracle, fm):
    """k_encode_l0, k_encode_l1p, k_encode_l2p; k_encode_l1pw and the level-2 kernel behind a warm window"""
    family, (lvl, warm) = fm
    single_calls(torch, ctx, oracle, items_of(oracle, family, lvl), lvl, warm)


@pytest.mark.parametrize("fm", families(ec.EXTENDED), ids=fm_id)
def test_extended_levels(torch, ctx, oracle, fm):
    family, (lvl, warm) = fm
    single_calls(torch, ctx, oracle, items_of(oracle, family, lvl), lvl, warm)


@pytest.mark.parametrize("fm", families([(1, 0), (2, 0)]), ids=fm_id)
def test_one_parser_kernels(torch, ctx, oracle, fm):
    """k_encode_l1 / k_encode_l2_t<0, false>: what runs where the LDS-order probe's verdict is "does not hold" (forced here)"""
    family, (lvl, _) = fm
    try:
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_order(0)
        assert (zz.lib.zz_debug_l1_kernel if lvl == 1 else zz.lib.zz_debug_l2_kernel)(ctx._h) == 1
        single_calls(torch, ctx, oracle, items_of(oracle, family, lvl), lvl, 0)
    finally:
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


@pytest.mark.parametrize("fm", families([(1, 0), (2, 0), (3, 0)]), ids=fm_id)
def test_rerun_after_a_reported_violation(torch, ctx, oracle, fm):
    """every call reports a violated LDS order (forced through the kernel's own report path) and runs again on the one-parser
    kernels, into the same destination with the same capacity. The items: three packets and a byte at every length, the tiny
    packets, every third tipping input."""
    family, (lvl, _) = fm
    items = items_of(oracle, family, lvl)
    items = items[1::3] if family == "tipping" else [it for it in items if it[0][1] in (3 * it[2] + 1, 4 * it[2] + 1)]
    assert len(items) >= 15

    def force():
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1          # (asking for the verdict runs the probe again)
        zz.lib.zz_debug_force_lds_violation(1)
    try:
        single_calls(torch, ctx, oracle, items, lvl, 0, before_each=force)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 0              # the last call's violation was seen
    finally:
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


def shard_calls(torch, ctx, oracle, items, lvl, warm, halo):
    """encode_shard per item against the oracle's packets. halo False: the whole input as a shard that is not the last, so that
    its last packet is not final either. halo True: everything behind the first packet, as the last shard, with the first packet
    as its halo."""
    if halo:
        items = [it for it in items if len(it[1]) > it[2]]
    caps = [zz.bound(len(d), ec.DEFLATE, lvl, P) for _, d, P, _ in items]
    s = Streams(torch, items, caps)
    bad = []
    ctx.set_extended_levels(lvl > 3)
    ctx.set_warm_window(warm)
    try:
        for i, (label, d, P, fmt) in enumerate(items):
            skip = P if halo else 0
            try:
                s.lens[i], _ = ctx.encode_shard(s.source(i) + skip, len(d) - skip, s.dest(i), caps[i], halo=skip, is_last=halo, checksum=fmt,
                                                level=lvl, packet_size=P)
            except zz.ZzFlateError as e:
                bad.append((label, "encode_shard raised", str(e)))
                continue
            if ctx.verify_last() != (0, None):
                bad.append((label, "verify_last"))
    finally:
        ctx.set_warm_window(0)
        ctx.set_extended_levels(False)
    streams, touched = s.collect()
    bad += [(t, "wrote outside its destination") for t in touched]
    for (label, d, P, _), got in zip(items, streams):
        want = b"".join(ec.oracle_packet(oracle, d, lvl, off, ln, final and halo, warm)
                        for off, ln, final in ec.packets(len(d), P) if off >= (P if halo else 0))
        if got != want:
            bad.append((label, "shard", len(got), len(want)))
    assert items and bad == [], (lvl, warm, halo, len(bad), bad[:8])


@pytest.mark.parametrize("fm", families(ec.COLD), ids=fm_id)
def test_shard_that_is_not_the_last(torch, ctx, oracle, fm):
    family, (lvl, warm) = fm
    shard_calls(torch, ctx, oracle, items_of(oracle, family, lvl), lvl, warm, False)


@pytest.mark.parametrize("fm", families([(1, 32768), (2, 32768), (3, 32768), (6, 0)]), ids=fm_id)
def test_shard_with_halo(torch, ctx, oracle, fm):
    family, (lvl, warm) = fm
    shard_calls(torch, ctx, oracle, items_of(oracle, family, lvl), lvl, warm, True)


@pytest.mark.parametrize("fm", families(ec.COLD), ids=fm_id)
def test_batch_at_exact_capacities(torch, ctx, oracle, fm):
    """all items of a family in encode_batch calls, one per container, every destination exactly as long as the oracle's stream:
    where a packet's slot is sized by the packet's own length and the item's room by the byte"""
    family, (lvl, _) = fm
    bad = []
    for fmt in range(3):
        items = [(label, d, P, fmt) for label, d, P, _ in items_of(oracle, family, lvl)]
        want = [oracle.encode_packets(d, fmt, lvl, P) for _, d, P, _ in items]
        s = Streams(torch, items, [len(w) for w in want])
        for size in sorted({it[2] for it in items}):                   # (a batch has one packet size)
            ids = [i for i, it in enumerate(items) if it[2] == size]
            lens = ctx.encode_batch([(s.source(i), len(items[i][1])) for i in ids], [(s.dest(i), len(want[i])) for i in ids], fmt, lvl, size)
            for i, w in zip(ids, lens):
                s.lens[i] = w or 0
                if w is None:
                    bad.append((items[i][0], fmt, "did not fit"))
        streams, touched = s.collect()
        bad += [(t, fmt, "wrote outside its destination") for t in touched]
        bad += [(it[0], fmt, "batch", len(got)) for it, got, exp in zip(items, streams, want) if got != exp]
        bad += [(b, fmt) for b in s.decode_batch(ctx)]
    assert bad == [], (family, lvl, len(bad), bad[:8])


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_batch_of_every_length(torch, ctx, oracle, family, lvl):
    """one input of every length of the list as the items of one batch, in packets of 4096, destinations exact"""
    P, fmt = 4096, lvl % 3
    gen = ec.high if family == "high" else ec.uniform
    items = [(L, gen(L, 3), P, fmt) for L in ec.LENGTHS + [3 * 4096 + 1, ec.MAX_N]]
    want = [oracle.encode_packets(d, fmt, lvl, P) for _, d, _, _ in items]
    s = Streams(torch, items, [len(w) for w in want])
    lens = ctx.encode_batch([(s.source(i), len(items[i][1])) for i in range(len(items))],
                            [(s.dest(i), len(want[i])) for i in range(len(items))], fmt, lvl, P)
    s.lens = [w or 0 for w in lens]
    streams, touched = s.collect()
    bad = [(t, "wrote outside its destination") for t in touched]
    bad += [(it[0], "batch", w) for it, got, exp, w in zip(items, streams, want, lens) if w is None or got != exp]
    bad += s.decode_batch(ctx)
    assert bad == [], (family, lvl, bad[:8])


@pytest.mark.parametrize("lvl", [1, 2])
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_members(torch, ctx, oracle, family, lvl):
    """blocked gzip files of blocks that do not compress: byte for byte the format rule's file (tests/members_write_cases.py), in
    which no member is longer than its stored form"""
    gen = ec.high if family == "high" else ec.uniform
    for n, B, P in ((ec.MAX_N, mw.BLOCK, 32768), (3 * 4096 + 1, 4096, 4096), (20000, 777, 300)):
        d = gen(n)
        want, offsets, stored = mw.expected(oracle, d, lvl, B, P, True)
        assert lvl != 1 or all(stored[:n // B])            # nine bits a byte, or 5.5 % growth: every full block falls back
        cap = zz.members_bound(n, B, P)
        dst = torch.full((cap + GAP,), 0xA5, dtype=torch.uint8, device="cuda")
        src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
        w = ctx.encode_members(src, n, dst, cap, lvl, B, P)
        host = dst.cpu().numpy().tobytes()
        assert host[:w] == want and w <= cap and host[cap:] == b"\xA5" * GAP, (family, lvl, n, B, P, w, len(want))
        assert ctx.last_encode_members_stats() == (len(stored), sum(stored))
        for j, (_, size) in enumerate(mw.members_of(want[:offsets[-1]])):
            assert size <= 26 + mw.stored_stream_bytes(min(B, n - j * B), P)
        back = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
        assert ctx.decode_members(dst, w, back, n + 1) == n and back[:n].cpu().numpy().tobytes() == d


@pytest.mark.parametrize("lvl", [0, 2, 3])
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_ranges(torch, ctx, oracle, family, lvl):
    """the reference's own split into 1, 2 and 3 ranges, one wavefront each, every range's blocks stored or nearly so"""
    gen = ec.high if family == "high" else ec.uniform
    bad = []
    for i, n in enumerate([1, 2, 17, 299, 300, 301, 1000, 4097, 32768, 65535, 65536, 65537, ec.MAX_N]):
        d, fmt = gen(n, 4), i % 3
        src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
        cap = 2 * n + 4096
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        for count in (1, 2, 3):
            want = oracle.encode_ranges(d, fmt, lvl, count) if n >= 100 * count else oracle.encode(d, fmt, lvl)
            assert ec.inflates(want, d, fmt)
            w = ctx.encode_ranges(src, n, dst, cap, count, fmt, lvl)
            if dst[:w].cpu().numpy().tobytes() != want:
                bad.append((n, fmt, count, w, len(want)))
    assert bad == [], (family, lvl, bad)
