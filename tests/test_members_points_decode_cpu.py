"""The decode through a member point index, on the CPU: tests/cxx/members_points_decode_harness.cpp restates
zz_decode_members_points_device on the host -- the check of the rows, descriptors and batches, phase 1 with the member's origin, the
rounds, the sums, the verdict's runs and tree, the serial tail -- with the rules of zzflate_amd/csrc/zz_inflate_core.h (zi_mpd_*), built
with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access bounds-checked; out of range aborts), with ONE lane and with 64
simulated lanes. The yardstick is zlib's own member loop (members_cases.yardstick, members_cases.produced, through
members_points_decode_cases.expected): the rows decide speed, never the result. Every call also holds the harness's host loops to
their iteration caps and the bytes behind `cap` to what they were."""
import os

import pytest

import members_cases as mc
import members_find_cases as fc
import members_points_cases as C
import members_points_decode_cases as DC

FILES = DC.files()
DAMAGED = C.damaged_cases()


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return C.build_harness(tmp_path_factory.mktemp("members_points_for_decode"))


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    return DC.build_harness(tmp_path_factory.mktemp("members_points_decode"))


@pytest.fixture(scope="module")
def rows_of(H):
    memo = {}

    def get(f, chunk=1000, spacing=1):
        if (f, chunk, spacing) not in memo:
            memo[f, chunk, spacing] = C.h_index(H, f, chunk, spacing)
        return memo[f, chunk, spacing]
    return get


# ---- 1. the shapes the list was chosen for, asserted on the rows before anything relies on them -------------------------------------------
def test_the_shapes_hold_what_the_tests_rely_on(rows_of):
    for name in DC.PLAIN:
        rows = rows_of(FILES[name]).rows
        segs = DC.segments(rows)
        if name in C.LARGE_MEMBERS:
            assert 16 <= len(segs) <= 92 and max(n for _, n in segs) <= 4064, (name, len(segs), max(n for _, n in segs))
            assert DC.batches(rows, 8192) >= 10, (name, DC.batches(rows, 8192))            # (10 .. 24: 168,100 bytes cannot take fewer than 21)
        assert DC.all_dealt(rows, rows[-1][1], 8192), name
    stored = DC.segments(rows_of(FILES[DC.STORED]).rows)
    assert max(n for _, n in stored) == 70000 and [m for m, n in stored if n > 8192] == [1]
    planted = sorted(max(n for _, n in DC.segments(rows_of(f).rows)) for f in C.planted_cases().values())
    assert planted[0] == 13852 and planted[-1] == 20994, planted
    for name, f in FILES.items():
        if name != DC.STORED:
            assert max(n for _, n in DC.segments(rows_of(f, 4096).rows)) <= 20994, name
        assert DC.batches(rows_of(f).rows, 0) == 1, name


# ---- 2. every file, every index of it: the yardstick's bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILES))
def test_valid_and_planted_files_equal_the_yardstick(D, rows_of, name):
    f = FILES[name]
    want = mc.yardstick(f)
    for chunk in DC.CHUNKS:
        for spacing in DC.SPACINGS:
            rows = rows_of(f, chunk, spacing).rows
            for batch in DC.BATCHES:
                r = DC.h_decode(D, f, rows, len(want), batch)
                assert r.verdict() == (DC.OK, want), (chunk, spacing, batch)
                dealt = DC.all_dealt(rows, len(want), batch)
                assert (r.proven == r.members and r.serial == 0) == dealt, (chunk, spacing, batch, r.proven, r.members)
                if dealt:
                    assert r.batches == DC.batches(rows, batch), (chunk, spacing, batch)


def test_pointers_reach_four_batches_back(D, rows_of):
    f = FILES[DC.NEAR]
    rows = rows_of(f).rows
    r = DC.h_decode(D, f, rows, rows[-1][1], 8192)
    assert r.serial == 0 and r.pending > 0 and r.rounds >= 1
    assert 32700 // 8192 + 1 >= 4 and max(n for _, n in DC.segments(rows)) <= 8192


def test_the_stored_member_takes_the_mstar_route(D, rows_of):
    f = FILES[DC.STORED]
    rows = rows_of(f).rows
    r = DC.h_decode(D, f, rows, rows[-1][1], 8192)
    assert r.verdict() == (DC.OK, mc.yardstick(f)) and (r.members, r.proven, r.serial) == (3, 1, 1)
    r = DC.h_decode(D, f, rows, rows[-1][1], 0)
    assert r.verdict() == (DC.OK, mc.yardstick(f)) and (r.members, r.proven, r.serial, r.batches) == (3, 3, 0, 1)


@pytest.mark.parametrize("name", C.SMALL + ("two large members",))
def test_sixty_four_lanes(D, rows_of, name):
    f = FILES[name]
    rows = rows_of(f).rows
    for batch in (0, 8192):
        one, many = DC.h_decode(D, f, rows, rows[-1][1], batch, 1), DC.h_decode(D, f, rows, rows[-1][1], batch, 64)
        assert many.verdict() == (DC.OK, mc.yardstick(f))
        assert (many.proven, many.batches, many.pending, many.rounds, many.serial) == (one.proven, one.batches, one.pending, one.rounds, one.serial)


# ---- 3. files zlib refuses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_files(D, H, rows_of, name):
    f, index_rc = DAMAGED[name]
    good, ms = C.three_large()
    good_rows = rows_of(good).rows
    own = C.h_index(H, f, 1000) if f else None
    for rows in ([good_rows] + ([own.rows] if own is not None and own.rc == C.OK else [])):
        for batch in (0, 8192):
            r = DC.h_decode(D, f, rows, len(mc.yardstick(good)) + 7, batch)
            assert r.verdict() == (DC.DATA, None), (name, batch)
    if name.startswith("CRC-32 wrong"):
        k = ("the first", "the middle", "the last").index(name[len("CRC-32 wrong in "):-len(" member")])
        assert own.rc == C.OK == index_rc
        r = DC.h_decode(D, f, own.rows, len(mc.yardstick(good)), 8192)
        assert (r.members, r.proven, r.serial) == (3, k, 1), "exactly the members in front of the damaged one are proven"


def test_truncation_at_every_byte(D, H):
    whole, _ = fc.small_three()
    rows = C.h_index(H, whole, 64).rows
    cap = len(mc.yardstick(whole))
    for f in C.truncations():
        assert DC.h_decode(D, f, rows, cap).verdict() == (DC.DATA, None), len(f)
        own = C.h_index(H, f, 64)
        if own.rc == C.OK:
            assert DC.h_decode(D, f, own.rows, cap).verdict() == (DC.DATA, None), len(f)


@pytest.mark.parametrize("dist", (1, 300, 3000))
def test_a_distance_in_front_of_the_member_is_an_error_not_a_pending_byte(D, H, dist):
    """the case the origin rule exists for: member 2's trailer holds the CRC-32 of the WRONG bytes, copied from member 1 -- a decoder
    that counts positions from the file's start accepts it; zlib answers "invalid distance too far back" """
    f, first = C.origin_case(dist)
    own = C.h_index(H, f, 1000)
    assert own.rc == C.OK and own.members == 2, "the index call judges no distance"
    for batch in (0, 8192, 1024):
        r = DC.h_decode(D, f, own.rows, len(first) + 10, batch)
        assert r.verdict() == DC.expected(f, len(first) + 10) == (DC.DATA, None), batch
        if batch != 1024:                                         # (at 1,024 member 1 holds a longer segment: it is m*)
            assert (r.members, r.proven, r.serial) == (2, 1, 1), batch


# ---- 4. rows that lie -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.LIES)
def test_lying_rows_change_nothing_but_the_path(D, rows_of, kind):
    f = FILES["three large members"]
    want = mc.yardstick(f)
    rows = rows_of(f).rows
    other = rows_of(FILES["two large members"]).rows
    lied = C.lie(rows, kind, other)
    assert lied != rows
    for batch in (0, 8192):
        r = DC.h_decode(D, f, lied, len(want), batch)
        assert r.verdict() == (DC.OK, want), (kind, batch)
        assert r.serial == 1 and r.proven < 3, (kind, batch, "the stats show the serial tail")
    for few in ([], rows[:1], rows[:2], rows[1:], [[0, 0], [8 * len(f), len(want)]]):
        assert DC.h_decode(D, f, few, len(want)).verdict() == (DC.OK, want)


# ---- 5. caps --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("three large members", "large members, an empty member and bgzip's last member", DC.STORED,
                                  "a member file stored in the middle member"))
def test_caps_around_every_member_boundary(D, rows_of, name):
    f = FILES[name]
    rows = rows_of(f).rows
    for cap in DC.caps_swept(f):
        for batch in (0, 8192):
            assert DC.h_decode(D, f, rows, cap, batch).verdict() == DC.expected(f, cap), (cap, batch)


def test_a_damaged_member_short_of_room(D, rows_of):
    """where a member is damaged AND short of room the yardstick needs `produced`: the bytes pass the room before the CRC is read"""
    f, _ = DAMAGED["CRC-32 wrong in the middle member"]
    good, ms = C.three_large()
    rows = rows_of(good).rows
    b = DC.boundaries(good)
    for cap in (b[1] + 5, b[2] - 2, b[2]):                        # (not b[2] - 1: `produced` counts the bytes zlib hands out in front of its check)
        want = DC.expected(f, cap)
        assert want[0] == (DC.DATA if cap == b[2] else DC.NOSPACE)
        assert DC.h_decode(D, f, rows, cap, 8192).verdict() == want, cap


# ---- 6. the stand-alone program under the address sanitizer ---------------------------------------------------------------------------------
def test_stand_alone_sanitizer_run(rows_of, tmp_path):
    import zlib
    exe = DC.build_main(tmp_path)
    for k, name in enumerate(("two large members", DC.STORED, DC.NEAR, "a member file stored in the first member")):
        f = FILES[name]
        want = mc.yardstick(f)
        path, rpath = os.path.join(str(tmp_path), f"f{k}.gz"), os.path.join(str(tmp_path), f"f{k}.rows")
        with open(path, "wb") as fh:
            fh.write(f)
        DC.write_rows(rpath, rows_of(f).rows)
        for batch in (0, 8192):
            rc, n, crc, stats = DC.run_main(exe, path, rpath, batch, len(want))
            assert (rc, n, crc) == (0, len(want), zlib.crc32(want)), (name, batch)
        assert DC.run_main(exe, path, rpath, 8192, len(want) - 1)[0] == DC.NOSPACE, name
    f, first = C.origin_case(300)
    path, rpath = os.path.join(str(tmp_path), "origin.gz"), os.path.join(str(tmp_path), "origin.rows")
    with open(path, "wb") as fh:
        fh.write(f)
    DC.write_rows(rpath, rows_of(f).rows)
    rc, _, _, stats = DC.run_main(exe, path, rpath, 0, len(first) + 10)
    assert rc == DC.DATA and stats[:2] == [2, 1]
