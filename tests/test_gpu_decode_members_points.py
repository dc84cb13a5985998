"""zz_decode_members_points_device (Context.decode_members_points): files of large gzip members decoded with many wavefronts per
member from their member point index. The yardstick is Context.decode_members on the same bytes in the same test -- status, length,
bytes -- for true rows, thinned rows, no rows, lying rows, damaged files, the member that copies from in front of its first byte, and
caps around a member boundary with guard bytes behind `cap`. The rows come from the CPU harness of the index
(tests/cxx/members_points_harness.cpp, which test_gpu_members_points.py holds the device's index to). Every test makes a bounded
number of serial-path calls; the sweeps over every cap and every truncation are the CPU harness's (test_members_points_decode_cpu.py).
Needs a real MI355X: run with `-m gpu`."""
import pytest

import zzflate_amd as zz
import members_points_cases as C
import members_points_decode_cases as DC

pytestmark = pytest.mark.gpu
FILES = DC.files()
DAMAGED = C.damaged_cases()
GUARD = 64


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
    return C.build_harness(tmp_path_factory.mktemp("members_points_decode_gpu"))


@pytest.fixture(scope="module")
def rows_of(H):
    memo = {}

    def get(f, chunk=1000, spacing=1):
        if (f, chunk, spacing) not in memo:
            r = C.h_index(H, f, chunk, spacing)
            assert r.rc == C.OK
            memo[f, chunk, spacing] = r.rows
        return memo[f, chunk, spacing]
    return get


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def tensor_of(torch, rows):
    return torch.tensor([[a - (1 << 64) if a >> 63 else a, b] for a, b in rows], dtype=torch.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def yardstick(torch, ctx):
    """(status, bytes or None) of decode_members for (file, cap): computed once per pair, shared by the tests"""
    memo = {}

    def get(f, cap):
        if (f, cap) not in memo:
            buf = torch.full((cap + 1,), 0xEE, dtype=torch.uint8, device="cuda")
            try:
                n = ctx.decode_members(dev(torch, f), len(f), buf, cap)
                memo[f, cap] = (0, buf[:n].cpu().numpy().tobytes())
            except zz.ZzFlateError as e:
                memo[f, cap] = (e.code, None)
        return memo[f, cap]
    return get


def decode(torch, ctx, f, rows, cap, batch=0, src=None):
    """(status, bytes or None, stats) of decode_members_points into cap bytes; the GUARD bytes behind cap must stay what they were"""
    src = dev(torch, f) if src is None else src
    buf = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    points = None if rows is None else tensor_of(torch, rows)
    try:
        out = ctx.decode_members_points(src, points, cap, len(f), buf, batch)
        got = (0, out.cpu().numpy().tobytes())
    except zz.ZzFlateError as e:
        got = (e.code, None)
    assert buf[cap:].cpu().numpy().tobytes() == b"\xEE" * GUARD, "bytes behind cap were written"
    return got + (ctx.last_decode_members_points_stats(),)


@pytest.mark.parametrize("name", list(FILES))
def test_valid_and_planted_files_equal_decode_members(torch, ctx, rows_of, yardstick, name):
    f = FILES[name]
    src = dev(torch, f)
    for chunk in (1000, 4096):
        rows = rows_of(f, chunk)
        L = rows[-1][1]
        want = yardstick(f, L)
        assert want[0] == 0 and len(want[1]) == L
        for batch in (0, 8192):
            rc, out, stats = decode(torch, ctx, f, rows, L, batch, src)
            assert (rc, out) == want, (chunk, batch)
            members, proven, segments, batches, pending, rounds, serial = stats
            if DC.all_dealt(rows, L, batch):                      # the conditions the shapes were chosen for, asserted on the rows
                assert (proven, serial) == (members, 0), (chunk, batch, stats)
                assert (segments, batches) == (len(DC.segments(rows)), DC.batches(rows, batch)), (chunk, batch, stats)
            else:
                assert serial == 1 and proven < members, (chunk, batch, stats)


def test_the_stored_member_takes_the_mstar_route(torch, ctx, rows_of, yardstick):
    f = FILES[DC.STORED]
    rows = rows_of(f)
    assert max(n for _, n in DC.segments(rows)) == 70000
    rc, out, stats = decode(torch, ctx, f, rows, rows[-1][1], 8192)
    assert (rc, out) == yardstick(f, rows[-1][1]) and (stats[0], stats[1], stats[6]) == (3, 1, 1), stats


def test_pointers_reach_across_batches(torch, ctx, rows_of, yardstick):
    f = FILES[DC.NEAR]
    rows = rows_of(f)
    assert max(n for _, n in DC.segments(rows)) <= 8192 and DC.batches(rows, 8192) >= 20
    rc, out, stats = decode(torch, ctx, f, rows, rows[-1][1], 8192)
    assert (rc, out) == yardstick(f, rows[-1][1])
    assert stats[4] > 0 and stats[5] >= 1 and stats[6] == 0, stats


def test_thinned_rows_and_no_rows(torch, ctx, rows_of, yardstick):
    for name in ("two large members", "a member file stored in the middle member"):
        f = FILES[name]
        L = rows_of(f)[-1][1]
        rc, out, stats = decode(torch, ctx, f, rows_of(f, 1000, 32768), L)
        assert (rc, out) == yardstick(f, L) and stats[6] == 0, name
        before = ctx.last_members_points_stats()
        rc, out, stats = decode(torch, ctx, f, None, L)           # the call makes the index itself
        assert (rc, out) == yardstick(f, L) and stats[1] == stats[0] > 0 and stats[6] == 0, name
        assert ctx.last_members_points_stats() == before
        out = ctx.decode_members_points(dev(torch, f))            # cap from members_points
        assert out.cpu().numpy().tobytes() == yardstick(f, L)[1], name


@pytest.mark.parametrize("name", [n for n in DAMAGED if n != "the empty file"])
def test_damaged_files(torch, ctx, rows_of, yardstick, name):
    f, _ = DAMAGED[name]
    good, _ = C.three_large()
    rows = rows_of(good)
    cap = rows[-1][1] + 7
    want = yardstick(f, cap)
    assert want == (zz.E_DATA, None)
    for batch in (0, 8192):
        rc, out, stats = decode(torch, ctx, f, rows, cap, batch)
        assert (rc, out) == want, batch
    rc, out, stats = decode(torch, ctx, f, None, cap)
    assert (rc, out) == want
    if name.startswith("CRC-32 wrong"):
        k = ("the first", "the middle", "the last").index(name[len("CRC-32 wrong in "):-len(" member")])
        assert (stats[0], stats[1], stats[6]) == (3, k, 1), "exactly the members in front of the damaged one are proven"


def test_the_empty_file(torch, ctx):
    with pytest.raises(zz.ZzFlateError) as e:
        ctx.decode_members_points(dev(torch, b""), None, 16, 0)
    assert e.value.code == zz.E_DATA


def test_a_distance_in_front_of_the_member_is_an_error(torch, ctx, H, yardstick):
    f, first = C.origin_case(300)
    own = C.h_index(H, f, 1000)
    assert own.rc == C.OK and own.members == 2
    cap = len(first) + 10
    assert yardstick(f, cap) == (zz.E_DATA, None)
    for batch in (0, 8192):
        rc, out, stats = decode(torch, ctx, f, own.rows, cap, batch)
        assert (rc, out) == (zz.E_DATA, None), batch
        assert (stats[0], stats[1], stats[6]) == (2, 1, 1), stats


@pytest.mark.parametrize("kind", C.LIES)
def test_lying_rows_change_nothing_but_the_path(torch, ctx, rows_of, yardstick, kind):
    f = FILES["three large members"]
    rows = rows_of(f)
    L = rows[-1][1]
    lied = C.lie(rows, kind, rows_of(FILES["two large members"]))
    rc, out, stats = decode(torch, ctx, f, lied, L, 8192)
    assert (rc, out) == yardstick(f, L), kind
    assert stats[6] == 1 and stats[1] < 3, (kind, stats)


@pytest.mark.parametrize("name", list(FILES))
def test_five_caps(torch, ctx, rows_of, yardstick, name):
    """L, L - 1, one member boundary and that boundary +- 1, for every file of the list (each has two members or more): five calls
    of the yardstick and five of the call, each with one member's serial work at the most"""
    f = FILES[name]
    rows = rows_of(f)
    b = DC.boundaries(f)
    assert len(b) >= 3 and 0 < b[1]
    L = b[-1]
    src = dev(torch, f)
    for cap in (L, L - 1, b[1], b[1] - 1, b[1] + 1):
        rc, out, stats = decode(torch, ctx, f, rows, cap, 8192, src)
        assert (rc, out) == yardstick(f, cap), cap


def test_the_other_calls_stats_stay_what_they_were(torch, ctx, rows_of):
    f = FILES["two large members"]
    src = dev(torch, f)
    L = rows_of(f)[-1][1]
    buf = torch.empty(L, dtype=torch.uint8, device="cuda")
    ctx.decode_members(src, len(f), buf, L)
    ctx.members_find(src)
    ctx.members_points(src, 1000)
    before = (ctx.last_decode_members_stats(), ctx.last_members_find_stats(), ctx.last_members_points_stats(), ctx.last_decode_path(),
              ctx.last_decode_stats())
    for rows in (rows_of(f), None, rows_of(f)[:3]):
        decode(torch, ctx, f, rows, L, 8192, src)
    assert before == (ctx.last_decode_members_stats(), ctx.last_members_find_stats(), ctx.last_members_points_stats(), ctx.last_decode_path(),
                      ctx.last_decode_stats())
