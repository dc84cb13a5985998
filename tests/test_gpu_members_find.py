"""zz_members_find_device / zz_decode_members_found_device (Context.members_find, Context.decode_members_found): the members of any
member file found on the device. The index and the stats must be exactly the CPU harness's (tests/cxx/members_find_harness.cpp,
which test_members_find_cpu.py holds to the pure-Python restatement), the decode must equal the yardstick -- zlib's member loop,
members_cases.yardstick -- and Context.decode_members in bytes, code and length, between guard bytes, and reads through the found
index must return the right bytes. Needs a real MI355X: run with `-m gpu`."""
import ctypes

import pytest

import zzflate_amd as zz
import members_cases as mc
import members_find_cases as fc

pytestmark = pytest.mark.gpu
GUARD = 64
VALID = fc.valid_cases()
REFUSED = fc.refusal_cases()
SWEEP = [n for n in REFUSED if n.startswith("three small members cut")]
NAMED = [n for n in REFUSED if n not in SWEEP]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return fc.build_harness(tmp_path_factory.mktemp("members_find_gpu"))


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def found(torch, ctx, f, cap, src=None):
    """(status, decoded bytes or None, stats) of decode_members_found; the guard bytes around dst[0, cap) must be untouched"""
    src = dev(torch, f) if src is None else src
    buf = torch.full((cap + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    rc, out = 0, None
    try:
        out = ctx.decode_members_found(src, cap, len(f), buf[GUARD:GUARD + cap])
        out = out.cpu().numpy().tobytes()
    except zz.ZzFlateError as e:
        rc = e.code
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().tobytes()
    assert raw[:GUARD] == b"\xEE" * GUARD and raw[GUARD + cap:] == b"\xEE" * GUARD, "bytes outside the destination were written"
    return rc, out, ctx.last_members_find_stats()


def serial(torch, ctx, f, cap, src=None):
    """(status, decoded bytes or None) of decode_members: the call whose verdicts the new one must give"""
    src = dev(torch, f) if src is None else src
    buf = torch.full((max(cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    try:
        n = ctx.decode_members(src, len(f), buf, cap)
    except zz.ZzFlateError as e:
        return e.code, None
    return 0, buf[:n].cpu().numpy().tobytes()


def find(torch, ctx, f, limit=0, src=None):
    """(status, rows, stats) of members_find"""
    src = dev(torch, f) if src is None else src
    try:
        rows = ctx.members_find(src, limit, len(f)).cpu().tolist()
    except zz.ZzFlateError as e:
        return e.code, [], ctx.last_members_find_stats()
    return 0, rows, ctx.last_members_find_stats()


@pytest.mark.parametrize("name", list(VALID))
def test_valid_files(torch, ctx, H, name):
    f = VALID[name][0]
    src = dev(torch, f)
    want = mc.yardstick(f)
    assert want is not None
    for limit in (64, 4096, 0):
        h = fc.h_find(H, f, limit or fc.LIMIT_DEFAULT)
        rc, rows, stats = find(torch, ctx, f, limit, src)
        assert (rc, rows) == (h.rc, h.rows) == (0, h.rows), limit
        assert stats == (h.members, h.candidates, h.dropped, h.rounds), limit
    h = fc.h_find(H, f)
    rc, out, stats = found(torch, ctx, f, len(want), src)
    assert (rc, out) == (0, want)
    assert stats == (h.members, h.candidates, h.dropped, h.rounds)
    assert serial(torch, ctx, f, len(want), src) == (0, want)
    for cap in (len(want) - 1, 0):
        got = found(torch, ctx, f, cap, src)[:2]
        assert got == fc.verdict(want, cap) == serial(torch, ctx, f, cap, src), cap


def test_more_members_than_resident_wavefronts(torch, ctx):
    # 5,000 jobs for the 4,096 resident wavefronts of k_members_reach and k_inflate_items: the dealing counters are used
    parts = [mc.text(10 + k % 50, k) for k in range(5000)]
    ms = [mc.member(p, (1, 6)[k & 1]) for k, p in enumerate(parts)]
    f, want = b"".join(ms), b"".join(parts)
    rows, at, off = [], 0, 0
    for m, p in zip(ms, parts):
        rows.append([at, off]); at += len(m); off += len(p)
    rows.append([at, off])
    src = dev(torch, f)
    rc, got, stats = find(torch, ctx, f, 0, src)
    assert (rc, got) == (0, rows) and stats[0] == 5000 and stats[1] - stats[2] == 5000 and stats[3] == 1
    assert found(torch, ctx, f, len(want), src)[:2] == (0, want)


@pytest.mark.parametrize("name", NAMED)
def test_refusals(torch, ctx, H, name):
    f = REFUSED[name]
    src = dev(torch, f)
    assert found(torch, ctx, f, 40000, src)[:2] == (zz.E_DATA, None) == serial(torch, ctx, f, 40000, src)
    for limit in (64, 0):
        h = fc.h_find(H, f, limit or fc.LIMIT_DEFAULT)
        rc, rows, stats = find(torch, ctx, f, limit, src)
        assert (rc, rows) == (h.rc, h.rows)
        assert stats == (h.members, h.candidates, h.dropped, h.rounds)


def test_truncation_at_every_byte(torch, ctx):
    whole = dev(torch, fc.small_three()[0])
    for name in SWEEP:
        f = REFUSED[name]
        assert found(torch, ctx, f, 200, whole)[:2] == (zz.E_DATA, None) == serial(torch, ctx, f, 200, whole), name      # (src_len cuts the file)
        assert find(torch, ctx, f, 64, whole)[0] == zz.E_DATA, name
    f, ms = fc.small_three()
    for k in (1, 2, 3):                                            # a cut behind a whole member leaves a valid file
        part = b"".join(ms[:k])
        assert found(torch, ctx, part, 200, whole)[:2] == (0, mc.yardstick(part))


def test_bad_crc_in_front_of_a_member_that_overflows(torch, ctx):
    f, good, _ = fc.crc_damaged()
    want = mc.yardstick(good)
    rows, _ = fc.true_chain(good)
    cap = rows[2][1] + 10                                          # members 0 and 1 fit, member 2 does not
    assert found(torch, ctx, good, cap)[:2] == (zz.E_NOSPACE, None) == serial(torch, ctx, good, cap)
    assert found(torch, ctx, f, cap)[:2] == (zz.E_DATA, None) == serial(torch, ctx, f, cap)
    assert found(torch, ctx, f, len(want))[:2] == (zz.E_DATA, None)


def test_caps_around_every_member_edge(torch, ctx):
    f = VALID["FNAME, FCOMMENT, FHCRC and a non-BC FEXTRA"][0]
    src = dev(torch, f)
    want = mc.yardstick(f)
    rows, _ = fc.true_chain(f)
    for cap in [len(want), len(want) - 1, 0] + [r[1] + d for r in rows[1:-1] for d in (-1, 0, 1)]:
        assert found(torch, ctx, f, cap, src)[:2] == fc.verdict(want, cap) == serial(torch, ctx, f, cap, src), cap
    empty = mc.member(b"") + mc.member(b"", 0) + mc.EOF_BLOCK
    assert found(torch, ctx, empty, 0)[:2] == (0, b"")


def test_damaged_members_short_of_room_get_decode_members_verdict(torch, ctx):
    a, b, c = mc.text(300, 1), mc.text(900, 2), mc.text(500, 3)
    good = mc.member(a) + mc.member(b) + mc.member(c)
    start1 = len(mc.member(a))
    for pos in range(start1 + 12, start1 + len(mc.member(b)), 97):
        f = bytearray(good); f[pos] ^= 0x10
        f = bytes(f)
        src = dev(torch, f)
        for cap in (len(a) + 5, len(a) + 450, len(a) + len(b) + len(c)):
            assert found(torch, ctx, f, cap, src)[:2] == serial(torch, ctx, f, cap, src), (pos, cap)


def test_cap_none_measures_first(torch, ctx):
    f = VALID["python gzip.compress members"][0]
    want = mc.yardstick(f)
    out = ctx.decode_members_found(dev(torch, f))
    assert out.cpu().numpy().tobytes() == want


def test_size_protocol(torch, ctx):
    f = VALID["python gzip.compress members"][0]
    src = dev(torch, f)
    rows, _ = fc.true_chain(f)
    idx = torch.full((2 * len(rows),), -1, dtype=torch.int64, device="cuda")
    n = ctypes.c_uint64(0)
    for room in (0, len(rows) - 1):
        rc = zz.lib.zz_members_find_device(ctx._h, src.data_ptr(), len(f), 0, idx.data_ptr(), room, ctypes.byref(n), None)
        torch.cuda.synchronize()
        assert (rc, n.value) == (zz.E_NOSPACE, len(rows)) and bool((idx == -1).all()), "the count is set, nothing is written"
    rc = zz.lib.zz_members_find_device(ctx._h, src.data_ptr(), len(f), 0, idx.data_ptr(), len(rows), ctypes.byref(n), None)
    torch.cuda.synchronize()
    assert (rc, n.value) == (0, len(rows)) and idx.view(-1, 2).cpu().tolist() == rows


def test_reads_through_the_found_index(torch, ctx):
    f = VALID["FNAME, FCOMMENT, FHCRC and a non-BC FEXTRA"][0]
    src = dev(torch, f)
    want = mc.yardstick(f)
    index = ctx.members_find(src)
    rows = index.cpu().tolist()
    assert rows == fc.true_chain(f)[0]
    reads = [(r[1] - 50, 100) for r in rows[1:-1]] + [(0, 10), (len(want) - 20, 1000), (rows[1][1] - 5, rows[3][1] - rows[1][1] + 10)]
    outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _, n in reads]
    lens, status = ctx.decode_members_ranges(src, len(f), index, [a for a, _ in reads], [n for _, n in reads], outs)
    assert status == [0] * len(reads)
    assert all(o[:ln].cpu().numpy().tobytes() == want[a:a + n] for o, ln, (a, n) in zip(outs, lens, reads))
    # a damaged CRC does not show in the index; the read that touches the member sees it, the others are complete
    f, good, _ = fc.crc_damaged()
    src = dev(torch, f)
    want = mc.yardstick(good)
    index = ctx.members_find(src)
    rows = index.cpu().tolist()
    assert rows == fc.true_chain(good)[0]
    reads = [(10, 100), (rows[1][1] - 10, 100), (rows[1][1] + 10, 100), (rows[2][1] - 10, 100)]
    outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _, n in reads]
    lens, status = ctx.decode_members_ranges(src, len(f), index, [a for a, _ in reads], [n for _, n in reads], outs)
    assert status == [zz.E_DATA, zz.E_DATA, 0, 0]
    assert all(o[:ln].cpu().numpy().tobytes() == want[a:a + n] for o, ln, (a, n), s in zip(outs, lens, reads, status) if s == 0)


def test_the_other_last_state_is_left_alone(torch, ctx):
    blocked = mc.bgzf(mc.text(3000, 1)) + mc.bgzf(mc.text(900, 2)) + mc.EOF_BLOCK
    want = mc.yardstick(blocked)
    assert serial(torch, ctx, blocked, len(want)) == (0, want)

    def state():
        return (ctx.last_decode_members_stats(), ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_points_index_stats(),
                ctx.last_decode_members_ranges_stats(), ctx.last_decode_ranges_stats())
    before = state()
    assert before[0] == (3, 3, mc.BLOCKED)
    f = VALID["stored bytes that look like headers and like a member"][0]
    assert found(torch, ctx, f, len(mc.yardstick(f)))[0] == 0
    assert find(torch, ctx, f, 64)[0] == 0
    assert found(torch, ctx, REFUSED["a junk byte between members"], 40000)[0] == zz.E_DATA
    assert found(torch, ctx, f, 10)[0] == zz.E_NOSPACE
    assert state() == before
