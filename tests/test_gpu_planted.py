"""Planted copies at every position around the encoders' internal boundaries (tests/planted_cases.py; the guards that need no GPU
are in tests/test_planted_cases_cpu.py): every encoder form's stream equals oracle.encode_packets(d, fmt, lvl, P, warm) byte for
byte, and the same streams go back through the batch decoder and, with the index of the call that wrote them, through Context.decode.
The container format cycles with the case's index. Needs a real MI355X: run with `-m gpu`.

A test is one (mode, family, boundary) cell of geometry A -- a few hundred cases -- or one (mode, packet size, family) of
geometry B, whose inputs are a few KiB."""
import ctypes

import pytest

import planted_cases as pc
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
DECODE_EVERY = 8                       # every eighth case also through Context.decode with the call's own packet index

CELLS_A = pc.cells(pc.cases_a())
CELLS_B = {}                           # geometry B by (packet size, family)
for _P in pc.B_PACKETS:
    for _c in pc.cases_b(_P):
        CELLS_B.setdefault((_P, _c[0]), []).append(_c)
FAMILIES_A = {}                        # geometry A by family: what one encode_batch call takes
for (_fam, _), _cs in CELLS_A.items():
    FAMILIES_A.setdefault(_fam, []).extend(_cs)
COLD = [(1, 0), (2, 0), (3, 0)]
WARM = [(1, 258), (1, 32768), (2, 4096), (3, 32768)]
EXTENDED = [(4, 0), (5, 0), (6, 0)]


def mode_id(m):
    return f"level{m[0]}" + (f"-warm{m[1]}" if m[1] else "")


def cell_id(k):
    return f"{k[0]}-{k[1]}"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


class Streams:
    """the inputs of a list of cases back to back in one device buffer, destinations of `cap` bytes each in another"""

    def __init__(self, torch, geometry, cases):
        self.torch = torch
        self.P, self.n = pc.size_of(geometry)
        self.data = [pc.plant(c, self.n) for c in cases]
        self.fmt = [i % 3 for i in range(len(cases))]
        self.src = torch.frombuffer(bytearray(b"".join(self.data)), dtype=torch.uint8).cuda()
        self.cap = max(zz.bound(self.n, 1, lvl, self.P) for lvl in (1, 2, 3))
        self.dst = torch.zeros(len(cases) * self.cap, dtype=torch.uint8, device="cuda")
        self.lens = [0] * len(cases)

    def source(self, i):
        return self.src.data_ptr() + i * self.n

    def dest(self, i):
        return self.dst.data_ptr() + i * self.cap

    def streams(self):
        host = self.dst.cpu().numpy().tobytes()
        return [host[i * self.cap: i * self.cap + w] for i, w in enumerate(self.lens)]

    def decode_batch(self, ctx):
        """every stream through Context.decode_batch, one call per container format: the cases that did not come back"""
        torch, bad = self.torch, []
        out = torch.full((len(self.data) * (self.n + 1),), 0xEE, dtype=torch.uint8, device="cuda")
        for fmt in range(3):
            ids = [i for i in range(len(self.data)) if self.fmt[i] == fmt]
            if not ids:
                continue
            lens, status = ctx.decode_batch([(self.dest(i), self.lens[i]) for i in ids],
                                            [(out.data_ptr() + i * (self.n + 1), self.n + 1) for i in ids], fmt)
            bad += [(i, "decode_batch", s, w) for i, s, w in zip(ids, status, lens) if s != 0 or w != self.n]
        host = out.cpu().numpy().tobytes()
        for i, d in enumerate(self.data):
            if host[i * (self.n + 1): (i + 1) * (self.n + 1)] != d + b"\xEE":
                bad.append((i, "decode_batch bytes"))
        return bad


def single_calls(torch, ctx, oracle, geometry, cases, lvl, warm):
    """Context.encode per case against the oracle; every stream through decode_batch, every eighth through Context.decode"""
    s = Streams(torch, geometry, cases)
    bad = []
    one = torch.zeros(s.n + 1, dtype=torch.uint8, device="cuda")
    ctx.set_extended_levels(lvl > 3)
    ctx.set_warm_window(warm)
    try:
        for i in range(len(cases)):
            s.lens[i] = ctx.encode(s.source(i), s.n, s.dest(i), s.cap, s.fmt[i], lvl, s.P)
            if i % DECODE_EVERY == 0:
                w = ctx.decode(s.dest(i), s.lens[i], one, s.n + 1, s.fmt[i], s.P, ctx.packet_index())
                if w != s.n or one[:w].cpu().numpy().tobytes() != s.data[i]:
                    bad.append((cases[i], "decode"))
    finally:
        ctx.set_warm_window(0)
        ctx.set_extended_levels(False)
    for i, got in enumerate(s.streams()):
        if got != oracle.encode_packets(s.data[i], s.fmt[i], lvl, s.P, warm):
            bad.append((cases[i], "encode", s.fmt[i]))
    bad += [(cases[b[0]],) + b[1:] for b in s.decode_batch(ctx)]
    assert bad == [], (geometry, lvl, warm, len(bad), bad[:8])


@pytest.mark.parametrize("cell", [k for k in CELLS_A if k[0] != "lazy"], ids=cell_id)
@pytest.mark.parametrize("mode", COLD + WARM, ids=mode_id)
def test_single_calls(torch, ctx, oracle, mode, cell):
    """k_encode_l1p / k_encode_l2p, cold and with a warm window"""
    single_calls(torch, ctx, oracle, "A", CELLS_A[cell], *mode)


@pytest.mark.parametrize("cell", list(CELLS_A), ids=cell_id)
@pytest.mark.parametrize("mode", EXTENDED, ids=mode_id)
def test_extended_levels(torch, ctx, oracle, mode, cell):
    """k_l6_matches in front of the level-2 kernel: every family, the lazy choice on every lane of a block included"""
    single_calls(torch, ctx, oracle, "A", CELLS_A[cell], *mode)


@pytest.mark.parametrize("cell", [k for k in CELLS_B if k[1] == "pos"], ids=cell_id)
@pytest.mark.parametrize("mode", COLD + WARM + EXTENDED, ids=mode_id)
def test_short_packets(torch, ctx, oracle, mode, cell):
    """geometry B: three packets and a short fourth, every position around every packet's first block, target and edge"""
    single_calls(torch, ctx, oracle, cell[0], CELLS_B[cell], *mode)


@pytest.mark.parametrize("cell", [k for k in CELLS_B if k[1] != "pos"], ids=cell_id)
@pytest.mark.parametrize("mode", WARM + EXTENDED, ids=mode_id)
def test_short_packets_windows(torch, ctx, oracle, mode, cell):
    """geometry B with a window: distances up to the stream's start, and sources in the stream's first bytes probed from the
    second packet (the shape of test_warm_window_candidates_at_the_very_start_of_the_stream)"""
    single_calls(torch, ctx, oracle, cell[0], CELLS_B[cell], *mode)


@pytest.mark.parametrize("cell", [k for k in CELLS_A if k[0] != "lazy"], ids=cell_id)
@pytest.mark.parametrize("lvl", [1, 2])
def test_classic_one_parser_kernels(torch, ctx, oracle, lvl, cell):
    """k_encode_l1 / k_encode_l2_t<0, false>: what runs where the LDS-order probe's verdict is "does not hold" (forced here)"""
    try:
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_order(0)
        single_calls(torch, ctx, oracle, "A", CELLS_A[cell], lvl, 0)
    finally:
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


@pytest.mark.parametrize("items", [("A", f) for f in FAMILIES_A if f != "lazy"] + [(P, "pos") for P in pc.B_PACKETS], ids=cell_id)
@pytest.mark.parametrize("lvl", [1, 2, 3])
def test_batch_forms(torch, ctx, oracle, lvl, items):
    """all cases of a family as the items of encode_batch calls (one call per container format, which a call has one of): each
    item's stream is the oracle's, and decode_batch gives the inputs back"""
    geometry, fam = items
    cases = FAMILIES_A[fam] if geometry == "A" else CELLS_B[items]
    s = Streams(torch, geometry, cases)
    for fmt in range(3):
        ids = [i for i in range(len(cases)) if s.fmt[i] == fmt]
        lens = ctx.encode_batch([(s.source(i), s.n) for i in ids], [(s.dest(i), s.cap) for i in ids], fmt, lvl, s.P)
        assert None not in lens
        for i, w in zip(ids, lens):
            s.lens[i] = w
    bad = [(cases[i], s.fmt[i]) for i, got in enumerate(s.streams()) if got != oracle.encode_packets(s.data[i], s.fmt[i], lvl, s.P)]
    bad += [(cases[b[0]],) + b[1:] for b in s.decode_batch(ctx)]
    assert bad == [], (items, lvl, len(bad), bad[:8])


def shard_cases():
    """the cases whose copy reaches into the second packet of geometry A"""
    return [c for c in pc.cases_a() if c[2] + c[3] > pc.A_P]


@pytest.mark.parametrize("mode", [(2, 32768), (3, 32768), (6, 0)], ids=mode_id)
def test_shard_with_halo(torch, ctx, oracle, mode):
    """the second packet of geometry A alone through encode_shard with the first as its halo: backward extension across the
    packet's start and every window candidate come out of the halo. Against the oracle's packet (zzo_packet_warm)."""
    lvl, warm = mode
    cases = shard_cases()
    assert len(cases) > 1500
    s = Streams(torch, "A", cases)
    off, ln = pc.A_P, pc.A_N - pc.A_P
    raw = ctypes.create_string_buffer(2 * ln + 1024)
    bad = []
    ctx.set_extended_levels(lvl > 3)
    ctx.set_warm_window(warm)
    try:
        for i in range(len(cases)):
            s.lens[i], _ = ctx.encode_shard(s.source(i) + off, ln, s.dest(i), s.cap, halo=off, is_last=True, checksum=zz.Format.Deflate,
                                            level=lvl, packet_size=pc.A_P)
    finally:
        ctx.set_warm_window(0)
        ctx.set_extended_levels(False)
    for i, got in enumerate(s.streams()):
        w = oracle.L.zzo_packet_warm(lvl, s.data[i], off, ln, 1, raw, len(raw), warm)
        if got != raw.raw[:w]:
            bad.append(cases[i])
        if i % 97 == 0:             # and the oracle's packet is the tail of the oracle's stream
            assert oracle.encode_packets(s.data[i], 2, lvl, pc.A_P, warm).endswith(raw.raw[:w])
    assert bad == [], (mode, len(bad), bad[:8])
