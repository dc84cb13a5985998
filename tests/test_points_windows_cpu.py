"""The sidecar built on the device, on the CPU: tests/cxx/points_windows_harness.cpp restates the whole of zz_points_windows_device
on the host with the rules of zzflate_amd/csrc/zz_inflate_core.h -- the batches over a stage addressed by absolute position, the
carry taken from the next batch's first slot, ZI_RUN_POINT onto zi_out_segment, the rounds, the cut, the pieces of a segment longer
than the stage, the fold, zi_points_thin -- built with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every access bounds-checked;
out of range aborts), with ONE lane and with 64 simulated lanes. The yardstick is zz_points_windows_host (whose own yardstick is
zlib, in test_points_ranges_cases_cpu.py) and the bytes that were compressed. These are also the guards of the list the device
test runs (tests/points_windows_cases.py)."""
import ctypes
import subprocess
import zlib

import pytest
import torch

import zzflate_amd as zz

import points_cases as pc
import points_ranges_cases as prc
import points_windows_cases as pw


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return pw.build_harness(tmp_path_factory.mktemp("points_windows"))


def host_code(s, fmt, rows):
    """zz_points_windows_host's verdict on rows that may lie"""
    segments = max(len(rows) - 1, 1)
    win = (ctypes.c_uint8 * (segments * pw.WINDOW))()
    sums = (ctypes.c_uint32 * segments)()
    return zz.lib.zz_points_windows_host(s, len(s), fmt, pc.flat(rows), len(rows), win, sums)


def check_honest(H, c, lanes=1, with_dst=False):
    name, spacing, fine, stage = c
    s, fmt, data = pc.case(name)
    rows, dense = pw.as_lists(pw.rows_of(name, spacing)), pw.as_lists(pw.rows_of(name, 1))
    plan = pw.plan_of(c, with_dst)
    r = pw.h_build(H, s, fmt, rows, dense if fine else None, stage, len(data) if with_dst else None, lanes)
    assert r.rc == plan.code, pw.case_id(c)
    if r.rc != pw.OK:
        return
    assert (r.windows, r.sums) == pw.host_bytes(*pw.host_sidecar(name, spacing)), pw.case_id(c)
    assert (r.batches, r.low_bases, r.seams, r.pieces) == (plan.batches, plan.low_bases, plan.seams, plan.pieces), pw.case_id(c)
    if with_dst:
        assert r.out == data, pw.case_id(c)


@pytest.mark.parametrize("name", pw.STREAMS)
def test_the_harness_makes_the_host_builders_sidecar(H, name):
    for c in pw.cases():
        if c[0] == name:
            check_honest(H, c)


@pytest.mark.parametrize("name", pw.STREAMS)
def test_with_a_destination_the_stream_is_left_there(H, name):
    for c in pw.cases():
        if c[0] == name and c[1] in (4096, 1 << 40) and c[3] in (0, 40000, pw.TINY_STAGE):
            check_honest(H, c, with_dst=True)


@pytest.mark.parametrize("name", ["alice_mem1", "alice_flushes", "alice_gzip_header", "alice_raw", "empty_gzip", "one_zlib"])
def test_sixty_four_lanes(H, name):
    for c in pw.cases():
        if c[0] == name and c[1] == 4096 and c[3] in (0, 40000, pw.TINY_STAGE):
            check_honest(H, c, lanes=64)
            check_honest(H, c, lanes=64, with_dst=True)


@pytest.mark.parametrize("name", pw.STREAMS)
def test_thinning_a_dense_index_is_the_builder_at_that_spacing(H, name):
    dense_t = pw.rows_of(name, 1)
    dense = pw.as_lists(dense_t)
    for spacing in pc.SPACINGS + (7, 1000):
        want = pw.rows_of(name, spacing)
        got = zz.points_thin(dense_t, spacing)
        assert got.device.type == "cpu" and torch.equal(got, want), (name, spacing)
        assert torch.equal(zz.points_thin(got, spacing), got), "idempotent"
        thin = pw.as_lists(want)
        assert pw.h_thin(H, dense, spacing) == (0, thin, len(thin))
        assert pw.h_thin(H, dense, spacing, len(thin) - 1) == (pw.NOSPACE, [], len(thin))
        assert H.zpw_superset(pc.flat(thin), len(thin), pc.flat(dense), len(dense)) == 1
        if len(thin) > 2 and len(dense) > len(thin):
            holed = [r for r in dense if r != thin[len(thin) // 2]]
            assert H.zpw_superset(pc.flat(thin), len(thin), pc.flat(holed), len(holed)) == 0
        assert H.zpw_superset(pc.flat(thin), len(thin), pc.flat(dense[:-1]), len(dense) - 1) == 0, "the last rows differ"


def test_the_lists_guards():
    plans = {c: pw.plan_of(c) for c in pw.cases()}
    ok = {c: p for c, p in plans.items() if p.code == pw.OK}
    assert {c[0] for c in ok} == set(pw.STREAMS)
    for stage in pw.SMALL_STAGES + (pw.TINY_STAGE,):
        mine = [(c, p) for c, p in ok.items() if c[3] == stage]
        assert any(p.batches >= 3 for _, p in mine), stage
        for c, p in mine:                                   # a batch holds at most the stage: a stream of more than twice that has three
            if len(pc.case(c[0])[2]) > 2 * stage:
                assert p.batches >= 3, pw.case_id(c)
        assert any(p.seams for _, p in mine), stage
    assert any(u[0] % pw.WINDOW for c, p in ok.items() if c[3] == 40000 for u in p.units), "a base that is no multiple of 32 KiB"
    assert any(p.low_bases for p in ok.values()), "a batch but the first whose base lies below 32 KiB"
    tiny = [p for c, p in ok.items() if c[3] == pw.TINY_STAGE]
    assert tiny and all(p.low_bases >= 3 and p.seams for p in tiny), "several batches inside the first 32 KiB, slots across their seams"
    assert any(p.multi for c, p in ok.items() if c[2]), "a sidecar segment of several fine segments"
    assert any(p.pieces for p in ok.values()), "a sidecar segment longer than the stage, cut in pieces"
    assert any(p.code == pw.UNSUPPORTED for p in plans.values())
    flushes = pw.as_lists(pw.rows_of("alice_flushes", 1))
    assert any(a[1] == b[1] for a, b in zip(flushes, flushes[1:])), "empty segments"


@pytest.mark.parametrize("name", prc.LIE_CASES)
def test_lying_indexes_get_the_host_builders_verdict(H, name):
    s, fmt, _ = pc.case(name)
    for spacing in prc.LIE_SPACINGS[name]:
        rows = pw.as_lists(pw.rows_of(name, spacing))
        assert len(rows) >= 4
        for kind in prc.SHAPE_LIES + prc.SEGMENT_LIES:
            lied = pc.lie(rows, kind, len(s))
            want = host_code(s, fmt, lied)
            assert want == pw.DATA, (name, kind)
            for stage in (0, 40000):
                if stage == 0 or pw.longest(rows) < stage - 1:
                    assert pw.h_build(H, s, fmt, lied, None, stage).rc == want, (name, spacing, kind, stage)


@pytest.mark.parametrize("name", ["alice_l6", "alice_gzip_header", "alice_raw"])
def test_damaged_streams_get_the_host_builders_verdict(H, name):
    s, fmt, _ = pc.case(name)
    rows = pw.as_lists(pw.rows_of(name, 4096))
    seen = set()
    for bad in pc.flipped(s, count=25) + pc.truncated(s):
        want = host_code(bad, fmt, rows)
        seen.add(want)
        assert pw.h_build(H, bad, fmt, rows, None, 0).rc == want
        assert pw.h_build(H, bad, fmt, rows, None, pw.longest(rows)).rc == want     # (the smallest stage that is not E_UNSUPPORTED)
    assert pw.DATA in seen


@pytest.mark.parametrize("name", ["alice_l6", "mix_l6"])
def test_a_stream_refused_only_for_its_trailer(H, name):
    s, fmt, data = pc.case(name)
    rows, dense = pw.as_lists(pw.rows_of(name, 32768)), pw.as_lists(pw.rows_of(name, 1))
    for bad in pw.trailer_damaged(s, fmt):
        assert pc.zlib_verdict(bad, fmt) is None
        assert zlib.decompressobj(-15).decompress(bad[pc.header_len(bad, fmt):]) == data, "the blocks are intact"
        assert host_code(bad, fmt, rows) == pw.DATA
        assert pw.h_build(H, bad, fmt, rows, None, 0).rc == pw.DATA
        assert pw.h_build(H, bad, fmt, rows, dense, pw.longest(dense)).rc == pw.DATA


def test_a_stage_one_byte_short_is_unsupported(H):
    for name, spacing, fine in (("alice_mem1", 4096, False), ("alice_mem1", 4096, True), ("mix_l6", 32768, False)):
        s, fmt, _ = pc.case(name)
        rows, dense = pw.as_lists(pw.rows_of(name, spacing)), pw.as_lists(pw.rows_of(name, 1))
        need = pw.longest(dense if fine else rows)
        assert pw.h_build(H, s, fmt, rows, dense if fine else None, need).rc == pw.OK
        assert pw.h_build(H, s, fmt, rows, dense if fine else None, need - 1).rc == pw.UNSUPPORTED


def test_a_far_distance_in_a_batch_with_a_low_base_is_refused(H):
    """the hand-made stream of points_ranges_cases: its second segment begins at byte 10 with a match of distance 11. With a stage
    of 10 bytes that segment is a batch of its own whose base is 10: a decode that counted from the stage's first byte instead of
    the stream's would find a byte there."""
    raw, rows, _, _, _ = prc.hand_made()
    assert host_code(raw, pc.RAW, rows) == pw.DATA
    plan = pw.Plan(rows, None, 10)
    assert plan.code == pw.OK and plan.batches == 2 and plan.low_bases == 1
    for lanes in (1, 64):
        assert pw.h_build(H, raw, pc.RAW, rows, None, 10, lanes=lanes).rc == pw.DATA
        assert pw.h_build(H, raw, pc.RAW, rows, None, 0, lanes=lanes).rc == pw.DATA
        assert pw.h_build(H, raw, pc.RAW, rows, None, 10, cap=13, lanes=lanes).rc == pw.DATA


def test_argument_errors_of_the_harness_are_the_calls(H):
    s, fmt, data = pc.case("alice_l6")
    rows, dense = pw.as_lists(pw.rows_of("alice_l6", 32768)), pw.as_lists(pw.rows_of("alice_l6", 1))
    assert pw.h_build(H, s, fmt, rows, dense[:-1] + [[dense[-1][0], dense[-1][1] + 1]], 0).rc == pw.ARG
    assert pw.h_build(H, s, fmt, rows, None, pw.BATCH + 1).rc == pw.ARG
    assert pw.h_build(H, s, fmt, rows, None, 0, cap=len(data) - 1).rc == pw.NOSPACE


def test_stand_alone_with_address_and_undefined_sanitizers(tmp_path):
    """mix_l6 has blocks of more than 65,536 bytes: at that stage the verdict is E_UNSUPPORTED, so it runs once more at its longest block"""
    exe = pw.build_main(tmp_path)
    mix_need = pw.longest(pw.as_lists(pw.rows_of("mix_l6", 1)))
    seen = set()
    for name, spacing, stage in (("alice_mem1", 4096, pw.TINY_STAGE), ("mix_l6", 32768, 65536), ("mix_l6", 32768, mix_need)):
        s, fmt, _ = pc.case(name)
        path = tmp_path / (name + ".bin")
        path.write_bytes(s)
        out = subprocess.run([exe, str(path), str(fmt), str(spacing), str(stage), "1"], check=True, capture_output=True, text=True).stdout.split("\n")
        windows, sums = pw.host_sidecar(name, spacing)
        plan = pw.plan_of((name, spacing, True, stage))
        seen.add(plan.code)
        if plan.code != pw.OK:
            assert out[0].split()[0] == str(plan.code), name
            continue
        assert out[0].split() == ["0", str(sums.shape[0]), str(plan.batches), str(plan.pieces)], name
        wb = windows.numpy()
        for k, line in enumerate(out[1: 1 + sums.shape[0]]):
            h = 0xcbf29ce484222325
            for b in wb[k].tobytes():
                h = ((h ^ b) * 0x100000001b3) & ((1 << 64) - 1)
            assert line.split() == ["%08x" % (int(sums[k]) & 0xFFFFFFFF), "%016x" % h], (name, k)
    assert seen == {pw.OK, pw.UNSUPPORTED}
