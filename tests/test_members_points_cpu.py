"""The member point index, on the CPU: tests/cxx/members_points_harness.cpp restates zz_members_points_device on the host -- both
candidate lists, the jobs with their limits, the walk over members and blocks with its repair rounds, the rows -- with the rules of zzflate_amd/csrc/zz_inflate_core.h,
built with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access bounds-checked; out of range aborts), with ONE lane
and with 64 simulated lanes. The yardsticks are a pure-Python restatement of the definition (members_points_cases.Expect: the
members from zlib's own loop, every block boundary from the host builder at spacing 1) and zlib's verdict (members_cases.yardstick)."""
import os
import zlib

import pytest

import members_cases as mc
import members_find_cases as fc
import members_points_cases as C
import points_cases as pc

VALID = C.valid_cases()
PLANTED = C.planted_cases()
DAMAGED = C.damaged_cases()
FILES = {**VALID, **PLANTED}


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return C.build_harness(tmp_path_factory.mktemp("members_points"))


@pytest.fixture(scope="module")
def HP(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp("members_points_truth"))


@pytest.fixture(scope="module")
def expect(H, HP):
    memo = {}

    def get(name, chunk):
        if (name, chunk) not in memo:
            hc, bc = C.h_candidates(H, FILES[name], chunk)
            memo[name, chunk] = C.Expect(HP, FILES[name], hc, bc), hc, bc
        return memo[name, chunk]
    return get


@pytest.fixture(scope="module")
def rows_of(H):
    memo = {}

    def get(name, chunk=4096):
        if (name, chunk) not in memo:
            r = C.h_index(H, FILES[name], chunk)
            assert r.rc == C.OK
            memo[name, chunk] = r.rows
        return memo[name, chunk]
    return get


# ---- 1. guards on the list: no kernel, no harness rule involved -------------------------------------------------------------------------
def test_every_valid_file_passes_zlibs_member_loop():
    for name, f in FILES.items():
        assert mc.checked(f) is not None, name
        assert len(f) <= 100000, name
    for name, (f, _) in DAMAGED.items():
        assert mc.yardstick(f) is None, name
    for dist in (1, 300):
        f, first = C.origin_case(dist)
        assert len(first) > dist
        with pytest.raises(zlib.error, match="invalid distance too far back"):
            d = zlib.decompressobj(31)
            d.decompress(f)
            zlib.decompressobj(31).decompress(d.unused_data)


def test_the_cases_hold_what_they_are_built_for(expect):
    for name, large in C.LARGE_MEMBERS.items():
        E, _, _ = expect(name, 1000)
        assert all(E.inner_of[j] >= 8 for j in large), (name, E.inner_of)
    for name in PLANTED:
        for chunk in C.CHUNKS:
            E, _, _ = expect(name, chunk)
            assert E.dropped_blocks >= 1, (name, chunk)
            assert E.dropped_headers >= 1 or name == C.REPAIRED, (name, chunk)
    E, hc, bc = expect(C.ABSORBED, 1000)
    first = C.bit_of(E.rows[[i for i, r in enumerate(E.rows) if r[0] & C.START][1]][0])
    assert first in bc and first // 8000 >= 1 and not [b for b in bc if b // 8000 == first // 8000 and b < first], "the absorbed case"
    assert E.absorbed >= 1 and fc.true_chain(VALID[C.ABSORBED])[0][1][0] == 64000
    for d in (-1, 0, 1):
        chain = fc.true_chain(VALID[f"a member end {d:+d} bytes from a chunk edge"])[0]
        assert (chain[1][0], chain[2][0]) == (8000 + d, 16384 + d)
    E, _, _ = expect("two large members", 1000)
    assert any(C.bit_of(r[0]) % 8 for r in E.rows if r[0] & C.END), "a final block that ends in mid-byte"
    E, _, bc = expect("a stored member of more than 64 KiB", 1000)
    assert E.inner_of[1] == 0 and E.rows[-1][1] - 70000 > 0
    E, _, _ = expect("a one-block fixed member", 1000)
    f = VALID["a one-block fixed member"]
    at = fc.true_chain(f)[0][1][0]
    assert f[at + 10] & 7 == 3, "BFINAL 1, BTYPE 1"
    E, _, bc = expect("two large members", C.BIGGER_THAN_ANY)
    assert bc == [] and len(E.rows) == 4, "a chunk larger than the file: no block candidates"


# ---- 2. the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILES))
def test_rows_equal_the_restatement(H, expect, name):
    f = FILES[name]
    for chunk in C.CHUNKS + (C.BIGGER_THAN_ANY,):
        E, hc, bc = expect(name, chunk)
        results = []
        for limit in C.LIMITS:
            r = C.h_index(H, f, chunk, limit=limit)
            assert (r.rc, r.rows, r.out_len, r.entries) == (C.OK, E.rows, E.out_len, len(E.rows)), (chunk, limit)
            assert (r.members, r.header_candidates, r.block_candidates, r.dropped) == (E.members, len(hc), len(bc), E.dropped), (chunk, limit)
            assert r.entries <= C.bound(f, chunk)
            results.append(r)
        assert results[0].rounds >= results[2].rounds and results[0].jobs >= results[2].jobs, "a small limit only adds rounds"
        if chunk == 1000 and name in C.LARGE_MEMBERS:
            assert results[0].rounds > 1, "a limit of 64 bytes makes jobs of the true walk give up"
        if chunk == C.BIGGER_THAN_ANY:
            assert C.h_to_index(H, E.rows) == fc.true_chain(f)[0], "no block candidates: the index is the member finder's"


def test_a_gap_is_repaired_in_a_second_round(H, expect):
    f = PLANTED[C.REPAIRED]
    rounds = [C.h_index(H, f, chunk).rounds for chunk in C.CHUNKS]
    assert max(rounds) >= 2, rounds


@pytest.mark.parametrize("name", C.SMALL + tuple(PLANTED)[:1])
def test_sixty_four_lanes(H, name):
    f = FILES[name]
    want = mc.yardstick(f)
    for chunk in (1000, 4096):
        one = C.h_index(H, f, chunk)
        assert C.h_index(H, f, chunk, lanes=64).key() == one.key(), chunk
        assert C.h_index(H, f, chunk, limit=64, lanes=64).rows == one.rows, chunk
    assert one.out_len == len(want)


@pytest.mark.parametrize("name", list(FILES))
def test_thinning_keeps_start_and_end_rows(H, rows_of, name):
    f = FILES[name]
    dense = rows_of(name, 1000)
    for spacing in (4096, 32768, 1 << 40):
        r = C.h_index(H, f, 1000, spacing=spacing)
        assert r.rc == C.OK and [x for x in r.rows if x[0] & (C.START | C.END)] == [x for x in dense if x[0] & (C.START | C.END)]
        assert all(x in dense for x in r.rows)
        # the one rule, restated: an inner row stays iff it is the first at or behind the next multiple of `spacing`
        want, nxt = [], 0
        for bit, pos in dense:
            if bit & (C.START | C.END) or pos >= nxt:
                want.append([bit, pos])
                if not bit & C.END:
                    nxt = pos - pos % spacing + spacing
        assert r.rows == want, spacing
    assert C.h_index(H, f, 1000, spacing=1 << 40).entries == 2 * (len(fc.true_chain(f)[0]) - 1)


def test_the_size_protocol(H, rows_of):
    f, rows = FILES["two large members"], rows_of("two large members")
    for room in (0, len(rows) - 1):
        r = C.h_index(H, f, 4096, max_entries=room)
        assert (r.rc, r.entries, r.out_len) == (C.NOSPACE, len(rows), rows[-1][1])
    assert C.h_index(H, f, 4096, max_entries=len(rows)).rows == rows


@pytest.mark.parametrize("name", list(FILES))
def test_members_index_from_points(H, rows_of, name):
    for chunk in (64, 4096):
        assert C.h_to_index(H, rows_of(name, chunk)) == fc.true_chain(FILES[name])[0]


# ---- 3. files zlib refuses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", (1, 300))
def test_the_member_origin(H, dist):
    """member 2's first symbol copies from in front of its first byte: zlib says "invalid distance too far back". The index call
    counts and ISIZE agrees, so it succeeds: ZZ_OK is not a verdict on distances."""
    f, first = C.origin_case(dist)
    for chunk in (64, 4096):
        r = C.h_index(H, f, chunk)
        assert r.rc == C.OK and r.members == 2 and r.out_len == len(first) + 10
        assert C.h_to_index(H, r.rows)[1] == [len(C.big(first)), len(first)]


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_files(H, name):
    f, index_rc = DAMAGED[name]
    good, _ = C.three_large()
    r = C.h_index(H, f, 1000)
    assert r.rc == index_rc, "what the index call answers"
    assert C.h_index(H, f, 1000, limit=64).key()[:4] == r.key()[:4]
    if r.rc == C.OK:
        assert r.rows == C.h_index(H, good, 1000).rows, "the CRC-32 is not judged without bytes: the index is the good file's"


def test_truncation_at_every_byte(H):
    for f in C.truncations():
        assert mc.yardstick(f) is None
        assert C.h_index(H, f, 64).rc == C.DATA, len(f)
        assert C.h_index(H, f, 64, limit=64).rc == C.DATA, len(f)


@pytest.mark.parametrize("kind", C.LIES)
def test_rows_that_are_no_index(H, rows_of, kind):
    """the host helper judges the shape of what it is given: flags dropped, doubled or out of order give no pairs"""
    rows = C.lie(rows_of("three large members", 1000), kind, rows_of("two large members", 1000))
    got = C.h_to_index(H, rows)
    if kind in ("bit_plus_one", "out_plus_one", "rows_swapped"):
        assert got == fc.true_chain(FILES["three large members"])[0], "inner rows are not the helper's business"
    elif kind == "another_file":
        assert got == fc.true_chain(FILES["two large members"])[0]
    else:
        assert got == [], kind


# ---- 4. the stand-alone program under the address sanitizer ---------------------------------------------------------------------------------
def test_stand_alone_sanitizer_run(H, tmp_path):
    exe = C.build_main(tmp_path)
    todo = list(FILES.items()) + [(n, f) for n, (f, _) in DAMAGED.items()] + [("origin", C.origin_case(300)[0])]
    todo += [("cut %d" % len(f), f) for f in C.truncations()[::9]]
    for k, (name, f) in enumerate(todo):
        path = os.path.join(str(tmp_path), "case%d.bin" % k)
        with open(path, "wb") as fh:
            fh.write(f)
        for chunk, limit in ((1000, 0), (4096, 64)):
            found, pairs = C.run_main(exe, path, chunk, limit)
            h = C.h_index(H, f, chunk, limit=limit)
            assert found.key() == h.key(), (name, chunk)
            assert pairs == (len(C.h_to_index(H, h.rows)) if h.rc == C.OK else 0), (name, chunk)
