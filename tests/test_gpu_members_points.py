"""zz_members_points_device (Context.members_points): one index over the members of a file and the blocks inside them, built on the
device. Rows, decoded length and all five stats must be exactly the CPU harness's (tests/cxx/members_points_harness.cpp, which
test_members_points_cpu.py holds to the pure-Python restatement), for valid, planted, damaged and truncated files; and reads
through the index the host helper makes must return the right bytes. Needs a real MI355X: run with `-m gpu`."""
import pytest

import zzflate_amd as zz
import members_cases as mc
import members_find_cases as fc
import members_points_cases as C

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
VALID = C.valid_cases()
PLANTED = C.planted_cases()
DAMAGED = C.damaged_cases()
FILES = {**VALID, **PLANTED}


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
    return C.build_harness(tmp_path_factory.mktemp("members_points_gpu"))


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def rows_of(points):
    return [[a & M64, b] for a, b in points.tolist()]


def tensor_of(torch, rows):
    return torch.tensor([[a - (1 << 64) if a >> 63 else a, b] for a, b in rows], dtype=torch.int64).reshape(-1, 2)


def index(torch, ctx, f, chunk, spacing=1, src=None):
    """(status, rows, decoded length, stats) of members_points"""
    src = dev(torch, f) if src is None else src
    try:
        points, n = ctx.members_points(src, chunk, spacing, len(f))
    except zz.ZzFlateError as e:
        return e.code, [], 0, ctx.last_members_points_stats()
    return 0, rows_of(points), n, ctx.last_members_points_stats()


def serial(torch, ctx, f, cap, src=None):
    """(status, decoded bytes or None) of decode_members: the call that gives the verdict on a file's bytes"""
    src = dev(torch, f) if src is None else src
    buf = torch.full((max(cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    try:
        n = ctx.decode_members(src, len(f), buf, cap)
    except zz.ZzFlateError as e:
        return e.code, None
    return 0, buf[:n].cpu().numpy().tobytes()


@pytest.mark.parametrize("name", list(FILES))
def test_index_equals_the_harness(torch, ctx, H, name):
    f = FILES[name]
    src = dev(torch, f)
    for chunk in C.CHUNKS + (C.BIGGER_THAN_ANY,):
        h = C.h_index(H, f, chunk)
        rc, rows, n, stats = index(torch, ctx, f, chunk, 1, src)
        assert (rc, rows, n) == (h.rc, h.rows, h.out_len) == (0, h.rows, h.out_len), chunk
        assert stats == h.stats(), chunk
    h = C.h_index(H, f, 1000, spacing=32768)
    rc, rows, n, stats = index(torch, ctx, f, 1000, 32768, src)
    assert (rc, rows, n, stats) == (0, h.rows, h.out_len, h.stats())


def test_more_jobs_than_resident_wavefronts(torch, ctx):
    # 5,000 small members and two large ones at chunk 64: more jobs than the 4,096 resident wavefronts of k_members_points_reach, so
    # the dealing counter is used
    parts = [mc.text(10 + k % 50, k) for k in range(5000)]
    alice = mc.corpus("alice29.txt")
    f = C.big(alice[:40000]) + b"".join(mc.member(p, (1, 6)[k & 1]) for k, p in enumerate(parts)) + C.big(alice[40000:80000], 1)
    want = alice[:40000] + b"".join(parts) + alice[40000:80000]
    rc, rows, n, stats = index(torch, ctx, f, 64)
    assert (rc, n) == (0, len(want)) and stats[0] == 5002 and len(rows) > 2 * 5002 + 100 and stats[1] + stats[2] > 4096
    assert zz.members_index_from_points(tensor_of(torch, rows)).tolist() == fc.true_chain(f)[0]


@pytest.mark.parametrize("dist", (1, 300))
def test_the_member_origin(torch, ctx, H, dist):
    """the index counts and ISIZE agrees, so the call succeeds on a file zlib refuses for a distance: ZZ_OK is no verdict on the bytes"""
    f, first = C.origin_case(dist)
    for chunk in (64, 4096):
        h = C.h_index(H, f, chunk)
        assert index(torch, ctx, f, chunk) == (0, h.rows, len(first) + 10, h.stats())
    assert serial(torch, ctx, f, len(first) + 10) == (zz.E_DATA, None)


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_files(torch, ctx, H, name):
    f, index_rc = DAMAGED[name]
    for chunk in (1000, 4096):
        h = C.h_index(H, f, chunk)
        rc, rows, n, stats = index(torch, ctx, f, chunk)
        assert (rc, rows, n) == (h.rc, h.rows, h.out_len) and rc == index_rc and stats == h.stats(), chunk
    assert serial(torch, ctx, f, 40000) == (zz.E_DATA, None), "the decode call gives the verdict on the bytes"


def test_truncation_at_every_byte(torch, ctx, H):
    whole, _ = fc.small_three()
    src = dev(torch, whole)
    for f in C.truncations():
        assert index(torch, ctx, f, 64, 1, src)[0] == zz.E_DATA, len(f)                  # (src_len cuts the file)
    h = C.h_index(H, whole, 64)
    assert index(torch, ctx, whole, 64, 1, src) == (0, h.rows, h.out_len, h.stats())


def test_size_protocol(torch, ctx, H):
    import ctypes
    f = FILES["two large members"]
    src = dev(torch, f)
    h = C.h_index(H, f, 4096)
    buf = (ctypes.c_uint64 * (2 * len(h.rows)))(*([0xEEEE] * (2 * len(h.rows))))
    n, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for room in (0, len(h.rows) - 1):
        rc = zz.lib.zz_members_points_device(ctx._h, src.data_ptr(), len(f), 4096, 1, buf, room, ctypes.byref(n), ctypes.byref(total), None)
        assert (rc, n.value, total.value) == (zz.E_NOSPACE, len(h.rows), h.out_len) and all(v == 0xEEEE for v in buf), "the counts are set, nothing is written"
    rc = zz.lib.zz_members_points_device(ctx._h, src.data_ptr(), len(f), 4096, 1, buf, len(h.rows), ctypes.byref(n), ctypes.byref(total), None)
    assert (rc, n.value) == (0, len(h.rows)) and [[buf[2 * i], buf[2 * i + 1]] for i in range(n.value)] == h.rows


def test_reads_through_the_index_the_helper_makes(torch, ctx):
    f = FILES["FEXTRA, FNAME, FCOMMENT and FHCRC headers"]
    src = dev(torch, f)
    want = mc.yardstick(f)
    points, n = ctx.members_points(src, 4096)
    index_rows = zz.members_index_from_points(points)
    assert index_rows.tolist() == fc.true_chain(f)[0] and n == len(want)
    edges = [r[1] for r in index_rows.tolist()[1:-1]]
    reads = [(e - 2048, 4096) for e in edges] + [(0, 10), (len(want) - 20, 1000)]
    outs = [torch.zeros(k, dtype=torch.uint8, device="cuda") for _, k in reads]
    lens, status = ctx.decode_members_ranges(src, len(f), index_rows.cuda(), [a for a, _ in reads], [k for _, k in reads], outs)
    assert status == [0] * len(reads)
    assert all(o[:ln].cpu().numpy().tobytes() == want[a:a + k] for o, ln, (a, k) in zip(outs, lens, reads))


def test_the_other_last_state_is_left_alone(torch, ctx):
    blocked = mc.bgzf(mc.text(3000, 1)) + mc.bgzf(mc.text(900, 2)) + mc.EOF_BLOCK
    want = mc.yardstick(blocked)
    assert serial(torch, ctx, blocked, len(want)) == (0, want)
    plain = fc.valid_cases()["python gzip.compress members"][0]
    ctx.decode_members_found(dev(torch, plain))

    def state():
        return (ctx.last_decode_members_stats(), ctx.last_decode_path(), ctx.last_decode_stats(), ctx.last_points_index_stats(),
                ctx.last_members_find_stats(), ctx.last_decode_members_ranges_stats(), ctx.last_decode_ranges_stats())
    before = state()
    assert before[0] == (3, 3, mc.BLOCKED)
    assert index(torch, ctx, FILES[C.REPAIRED], 1000)[0] == 0
    assert index(torch, ctx, DAMAGED["one byte of garbage behind the first trailer"][0], 1000)[0] == zz.E_DATA
    assert state() == before
