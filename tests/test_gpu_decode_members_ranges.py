"""zz_decode_members_ranges_device / Context.decode_members_ranges and zz_members_index_device / Context.members_index: reads
of a blocked gzip (BGZF) file through its index, and the index made on the device. The yardstick for every read is
members_ranges_cases.Judge -- zlib's verdict on each member the index cuts out: a read whose members zlib accepts comes back
byte for byte, any other is E_DATA -- on the whole case list (good files, damaged files, lying indexes), all reads of a file in
one call and one read per call; then the index builder, the round trip with the writer, one decode per member, three waves,
and the context's other state. Needs a real MI355X: run with `-m gpu`."""
import ctypes
import random
import zlib

import pytest

import zzflate_amd as zz
import members_cases as mc
import members_ranges_cases as rc

pytestmark = pytest.mark.gpu
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
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def index_tensor(torch, idx):
    def i64(v):
        v %= 1 << 64
        return v - (1 << 64) if v >> 63 else v
    return torch.tensor([[i64(c), i64(u)] for c, u in idx], dtype=torch.int64).cuda()


def call(torch, ctx, file, idx, reads, src=None, index=None):
    """(return code, [(status, bytes or None)], stats) of one call. The destinations lie in one buffer, 32 guard bytes on both
    sides of each, every residue mod 16 among their addresses; the guards, and for a failed read the bytes behind cap, must be
    untouched -- and every byte of every destination where the index is no index."""
    src = dev(torch, file) if src is None else src
    index = index_tensor(torch, idx) if index is None else index
    offs, caps, size = rc.layout(reads, idx)
    buf = torch.full((size,), 0xEE, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lens, status = ctx.decode_members_ranges(src, len(file), index, [r[0] for r in reads], [r[1] for r in reads],
                                             [(buf.data_ptr() + o, cp) for o, cp in zip(offs, caps)], caps)
    err = zz.lib.zz_last_error()
    torch.cuda.synchronize()
    img = buf.cpu().numpy().tobytes()
    res, used = [], bytearray(size)
    for r, (o, cp) in enumerate(zip(offs, caps)):
        if status[r] == 0:
            assert lens[r] <= cp, (r, reads[r])
            res.append((0, img[o:o + lens[r]]))
            used[o:o + lens[r]] = b"\x01" * lens[r]
        else:
            assert lens[r] is None
            res.append((status[r], None))
            if rc.index_ok(file, idx):
                used[o:o + cp] = b"\x01" * cp
    stray = [i for i, (u, b) in enumerate(zip(used, img)) if not u and b != 0xEE]
    assert not stray, ("bytes outside the destinations were written", stray[:8])
    code = next((e for e in (rc.E_DATA, rc.E_UNSUPPORTED, rc.E_ARG, rc.E_NOSPACE) if e in status), 0)
    assert code == 0 or err.startswith(b"reads: ")             # a read's own failure is worded so, and does not raise
    return code, res, ctx.last_decode_members_ranges_stats()


def raw_call(torch, ctx, file, idx, reads):
    """the C entry point's own return code for a call (destinations of cap bytes each)"""
    src, index = dev(torch, file), index_tensor(torch, idx)
    offs, caps, size = rc.layout(reads, idx)
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    tab = torch.tensor([[r[0] - (1 << 64) if r[0] >> 63 else r[0] for r in reads], [r[1] - (1 << 64) if r[1] >> 63 else r[1] for r in reads],
                        [buf.data_ptr() + o for o in offs], caps], dtype=torch.int64).cuda()
    out = torch.zeros(len(reads), dtype=torch.int64, device="cuda")
    code = zz.lib.zz_decode_members_ranges_device(ctx._h, src.data_ptr(), len(file), index.data_ptr(), len(idx), len(reads), tab[0].data_ptr(),
                                                  tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), out.data_ptr(), None, None)
    torch.cuda.synchronize()
    return code, out.cpu().tolist()


CASES = rc.all_cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_all_reads_of_a_file_in_one_call(torch, ctx, case):
    name, file, idx, reads = CASES[case]
    J = rc.Judge(file, idx)
    want_code, want = J.call(reads)
    code, got, (dec, waves) = call(torch, ctx, file, idx, reads)
    for r, (w, g) in enumerate(zip(want, got)):
        assert w == g, (name, r, reads[r], w[0], g[0])
    assert code == want_code
    assert dec == J.decoded(reads) and waves == (1 if dec else 0)
    # the C call's own return code, and lengths without a status array
    code, lens = raw_call(torch, ctx, file, idx, reads)
    assert code == want_code
    assert lens == [len(b) if s == 0 else -1 for s, b in want]


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_one_read_per_call(torch, ctx, case):
    name, file, idx, reads = CASES[case]
    J = rc.Judge(file, idx)
    src, index = dev(torch, file), index_tensor(torch, idx)
    seen = set()
    for r in reads:
        if r in seen:
            continue
        seen.add(r)
        code, got, _ = call(torch, ctx, file, idx, [r], src, index)
        want = J.read(*r)
        assert got[0] == want and code == want[0], (name, r, want[0], got[0][0])


def member_loop_index(file):
    """the index by zlib's member loop"""
    idx, c, u, rest = [], 0, 0, file
    while rest:
        d = zlib.decompressobj(31)
        n = len(d.decompress(rest))
        assert d.eof
        idx.append((c, u))
        c += len(rest) - len(d.unused_data)
        u += n
        rest = d.unused_data
    return idx + [(c, u)]


def test_index_builder(torch, ctx):
    walked = [f for name, f, path in mc.path_cases() if path == mc.WALKED][0]
    files = [(name, f) for name, f, _ in rc.good_files()] + [("a stored blocked file in the middle (path 2)", walked)]
    for name, f in files:
        want = member_loop_index(f)
        got = ctx.members_index(dev(torch, f), len(f))
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(want), 2) and got.is_cuda, name
        assert [tuple(p) for p in got.cpu().tolist()] == want, name
    for name, f, idx in rc.good_files()[:5]:
        assert member_loop_index(f) == idx, name                  # (the case list's own indexes, where they cover the file)
    a, b = mc.text(3000, 1), mc.text(9000, 2)
    import gzip
    with pytest.raises(zz.ZzFlateError) as e:
        f = gzip.compress(a) + gzip.compress(b)
        ctx.members_index(dev(torch, f), len(f))
    assert e.value.code == zz.E_UNSUPPORTED
    with pytest.raises(zz.ZzFlateError) as e:
        f = mc.bgzf(a) + mc.member(b) + mc.bgzf(a)
        ctx.members_index(dev(torch, f), len(f))
    assert e.value.code == zz.E_UNSUPPORTED
    with pytest.raises(zz.ZzFlateError) as e:
        ctx.members_index(dev(torch, b""), 0)
    assert e.value.code == zz.E_DATA
    # one entry too few: the count is reported and nothing is written
    name, f, idx = rc.good_files()[1]
    out = torch.full((len(idx), 2), -7, dtype=torch.int64, device="cuda")
    n = ctypes.c_uint64(0)
    src = dev(torch, f)
    assert zz.lib.zz_members_index_device(ctx._h, src.data_ptr(), len(f), out.data_ptr(), len(idx) - 1, ctypes.byref(n), None) == zz.E_NOSPACE
    torch.cuda.synchronize()
    assert n.value == len(idx) and bool((out == -7).all())
    assert zz.lib.zz_members_index_device(ctx._h, src.data_ptr(), len(f), out.data_ptr(), len(idx), ctypes.byref(n), None) == 0
    assert [tuple(p) for p in out.cpu().tolist()] == idx


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("B,P", [(65280, 32768), (777, 300)])
def test_round_trip_with_the_writer(torch, ctx, level, B, P):
    data = (mc.corpus("lcet10.txt") + mc.corpus("plrabn12.txt") + mc.corpus("alice29.txt"))[:1000000]
    assert len(data) == 1000000
    src = dev(torch, data)
    cap = zz.members_bound(len(data), B, P, True)
    file = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    members = -(-len(data) // B)
    offs = torch.full((members + 1,), -1, dtype=torch.int64, device="cuda")
    w = ctx.encode_members(src, len(data), file, cap, level, B, P, True, offs)
    idx = zz.members_index_from_offsets(offs.cpu().tolist(), len(data), block_size=B, eof=True)
    index = ctx.members_index(file, w)
    assert [tuple(p) for p in index.cpu().tolist()] == idx
    rng = random.Random(1000 * level + B)
    reads = []
    for _ in range(256):
        n = rng.choice((1, 17, 4096, 70000, 3 * B + 5))
        reads.append((rng.randrange(len(data)), n))
    dsts = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _, n in reads]
    lens, status = ctx.decode_members_ranges(file, w, index, [r[0] for r in reads], [r[1] for r in reads], dsts)
    assert status == [0] * 256
    for (first, n), ln, d in zip(reads, lens, dsts):
        want = data[first:first + n]
        assert ln == len(want) and d[:ln].cpu().numpy().tobytes() == want, (first, n)
        assert bool((d[ln:] == 0xEE).all())


def test_one_decode_per_member(torch, ctx):
    name, file, idx = rc.good_files()[3]
    assert name == "300 members of 100 bytes"
    whole = mc.checked(file)
    src, index = dev(torch, file), index_tensor(torch, idx)
    rng = random.Random(3)
    u = idx[17][1]
    reads = [(u + rng.randrange(100), 1 + rng.randrange(40)) for _ in range(4096)]
    buf = torch.zeros(4096 * 48, dtype=torch.uint8, device="cuda")
    lens, status = ctx.decode_members_ranges(src, len(file), index, [r[0] for r in reads], [min(r[1], u + 100 - r[0]) for r in reads],
                                             [(buf.data_ptr() + 48 * r, 48) for r in range(4096)])
    assert status == [0] * 4096
    assert ctx.last_decode_members_ranges_stats() == (1, 1)
    img = buf.cpu().numpy().tobytes()
    for r, (first, n) in enumerate(reads):
        n = min(n, u + 100 - first)
        assert lens[r] == n and img[48 * r:48 * r + n] == whole[first:first + n], r
    L = len(whole)
    buf = torch.zeros(4096 * L, dtype=torch.uint8, device="cuda")
    lens, status = ctx.decode_members_ranges(src, len(file), index, [0] * 4096, [L] * 4096, [(buf.data_ptr() + L * r, L) for r in range(4096)])
    assert status == [0] * 4096 and lens == [L] * 4096
    assert ctx.last_decode_members_ranges_stats() == (300, 1)
    want = dev(torch, whole)
    assert bool((buf.view(4096, L) == want).all())


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_round_edges_of_the_planning_scans(torch, ctx, m):
    # k_mr_touched, k_mr_judge, k_mr_cut and k_members_pairs take 1024 members, ranks or reads a round: m tiny members, every one
    # touched, one read per member and three more, so that each carry is in use at the edge -- coverage (a read lies across member
    # 1023 | 1024), counts and rooms (every member), chunks (every read), and the damaged members in front of a rank (two members
    # with a flipped CRC: one in the first round, one that is the file's last member, which m = 1025 puts into the second)
    kinds = [rc.mem(mc.text(30 + 7 * k, k)) for k in range(16)]
    members = [kinds[(5 * j) % 16] for j in range(m)]
    for j in (5, m - 1):
        b = bytearray(members[j][0])
        b[-8] ^= 1
        members[j] = (bytes(b), members[j][1])
    file, idx = rc.build(members)
    u = [p[1] for p in idx]
    reads = [(u[j] + 3, 10, None) for j in range(m)] + [(u[1020], u[m] - u[1020], None), (u[6], u[m - 1] - u[6], None), (0, u[m], None)]
    J = rc.Judge(file, idx)
    want_code, want = J.call(reads)
    assert want_code == rc.E_DATA and [r for r, (s, _) in enumerate(want) if s != 0] == [5, m - 1, m, m + 2]
    code, got, (dec, waves) = call(torch, ctx, file, idx, reads)
    assert code == want_code and got == want
    assert (dec, waves) == (m, 1)
    # the index from the file alone: ISIZE is summed over the round edge (a flipped CRC does not change what a header announces)
    index = ctx.members_index(dev(torch, file), len(file))
    assert [tuple(p) for p in index.cpu().tolist()] == idx


def test_three_waves(torch, ctx):
    # the smallest shape with three waves: 3 x 64 MiB + 1 MiB of text, generated, written and compared on the device
    n = 3 * (64 << 20) + (1 << 20)
    data = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 5, 0, data, n)
    cap = zz.members_bound(n)
    file = torch.empty(cap, dtype=torch.uint8, device="cuda")
    members = -(-n // zz.MEMBERS_BLOCK)
    offs = torch.empty(members + 1, dtype=torch.int64, device="cuda")
    w = ctx.encode_members(data, n, file, cap, 1, offsets=offs)
    idx = zz.members_index_from_offsets(offs.cpu().tolist(), n)
    index = index_tensor(torch, idx)
    rng = random.Random(64)
    reads = [(0, n)] + [(k * (64 << 20) - 4096, 8192) for k in (1, 2, 3)] + [(rng.randrange(n - 4096), 4096) for _ in range(64)]
    dsts = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _, nb in reads]
    lens, status = ctx.decode_members_ranges(file, w, index, [r[0] for r in reads], [r[1] for r in reads], dsts)
    assert status == [0] * len(reads) and lens == [r[1] for r in reads]
    dec, waves = ctx.last_decode_members_ranges_stats()
    assert waves >= 3 and dec == members
    for (first, nb), d in zip(reads, dsts):
        assert torch.equal(d, data[first:first + nb]), (first, nb)


def test_other_state_is_left_alone(torch, ctx):
    data = mc.corpus("alice29.txt")
    src = dev(torch, data)
    enc = torch.zeros(zz.bound(len(data)), dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, len(data), enc, enc.numel(), zz.Format.Zlib, 2)
    back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    assert ctx.decode(enc, w, back, len(data), zz.Format.Zlib, index=ctx.packet_index()) == len(data)
    f = mc.bgzf(mc.text(3000, 1)) + mc.member(mc.text(100, 2))
    out = torch.zeros(3100, dtype=torch.uint8, device="cuda")
    assert ctx.decode_members(dev(torch, f), len(f), out, 3100) == 3100
    before = (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_members_stats(), ctx.verify_last())
    assert before[0] == zz.DECODE_INDEXED and before[2][2] == zz.MEMBERS_SERIAL
    name, file, idx = rc.good_files()[1]
    index = ctx.members_index(dev(torch, file), len(file))
    assert (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_members_stats(), ctx.verify_last()) == before
    code, got, _ = call(torch, ctx, file, idx, [(0, idx[-1][1], None)], index=index)
    assert code == 0 and got[0][1] == mc.checked(file)
    assert (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_decode_members_stats(), ctx.verify_last()) == before
