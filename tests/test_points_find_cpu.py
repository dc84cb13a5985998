"""The point index found in parallel, on the CPU: tests/cxx/points_find_harness.cpp restates zz_points_index_device on the host --
the finder chunk by chunk, the reach jobs with their limit, the links, the repair rounds, the rows, the trailer's place -- with
the rules of zzflate_amd/csrc/zz_inflate_core.h, built with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access
bounds-checked; out of range aborts), with ONE lane and with 64 simulated lanes. The yardsticks are the host builder's rows at
spacing 1 (every block of the true chain, through the points harness) and Python's zlib (tests/points_find_cases.py).

The cap on the clean list is "no dropped candidate": a header that passes the whole test where no block starts has not been seen
in about four million positions of three corpus files, so a clean stream's candidates all lie on its chain and one round does.
If a listed stream ever breaks that, the guard below names it and the stream is to be replaced; the cap is not raised."""
import os
import zlib

import pytest

import points_cases as pc
import points_find_cases as fc


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return fc.build_harness(tmp_path_factory.mktemp("points_find"))


@pytest.fixture(scope="module")
def HP(tmp_path_factory):
    return pc.build_harness(tmp_path_factory.mktemp("points_truth"))


@pytest.fixture(scope="module")
def truth(HP):
    """stream -> the host builder's rows at spacing 1: every block boundary of the true chain"""
    memo = {}

    def get(s, fmt):
        if (s, fmt) not in memo:
            rc, rows, n, entries = pc.h_build(HP, s, fmt, 1)
            assert rc == 0 and entries == len(rows)
            memo[s, fmt] = rows
        return memo[s, fmt]
    return get


def check_against_truth(f, T, s, fmt, chunk, data_len):
    """2. of the list: a subset of the true rows as exact pairs, first and last row and the length equal, and in every chunk c >= 1
    that holds the start of a non-final dynamic block of the true chain the row is the first such start"""
    assert f.rc == fc.OK and f.out_len == data_len and f.entries == len(f.rows)
    true_pairs = {tuple(r) for r in T}
    assert all(tuple(r) in true_pairs for r in f.rows)
    assert f.rows[0] == T[0] == [0, 0] and f.rows[-1] == T[-1]
    assert all(a[0] < b[0] for a, b in zip(f.rows, f.rows[1:]))
    d = fc.deflate_of(s, fmt)
    first_in_chunk = {}
    for b in fc.dynamic_starts(d, T):
        if b // (8 * chunk) >= 1:
            first_in_chunk.setdefault(b // (8 * chunk), b)
    inner = {r[0] // (8 * chunk): r[0] for r in f.rows[1:-1]}
    assert inner == first_in_chunk


# ---- 1. rule equality --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["alice_mem1", "merge_8000"])
@pytest.mark.parametrize("lanes", [1, 64])
def test_rules_agree_at_every_bit(H, truth, which, lanes):
    if which in fc.PLANTED:
        s, fmt, _, planted_bits = fc.planted(which)
    else:
        (s, fmt, _), planted_bits = pc.case(which), ()
    d = fc.deflate_of(s, fmt)
    cap = 8 * len(d)
    buf = (fc.u64 * cap)()
    n = fc.u64(0)
    bad = H.zpf_rules(d, len(d), lanes, buf, cap, fc.ctypes.byref(n))
    assert bad == 0, "zi_find_header, zi_run and the prefilter disagree somewhere"
    passing = [buf[i] for i in range(n.value)]
    starts = set(fc.dynamic_starts(d, truth(s, fmt)))
    assert starts <= set(passing), "a true non-final dynamic block start does not pass the test"
    assert all(p in passing for p in planted_bits)
    if not planted_bits:
        assert set(passing) == starts, "a header passes where no block of the clean stream starts: replace the stream (see the docstring)"


# ---- 2. the clean list and the cap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CLEAN)
def test_clean_streams(H, truth, name):
    s, fmt, data = pc.case(name)
    T = truth(s, fmt)
    for chunk in fc.chunks_of(name):
        f = fc.h_index(H, s, fmt, chunk)
        check_against_truth(f, T, s, fmt, chunk, len(data))
        assert (f.dropped, f.rounds) == (0, 1), (name, chunk, "the cap: no dropped candidate on the clean list")
        assert f.candidates == len(f.rows) - 1 and f.jobs == f.candidates
        assert f.entries <= len(s) // chunk + 2, "zz_points_index_bound"


@pytest.mark.parametrize("name", fc.SMALL)
def test_sixty_four_lanes(H, name):
    s, fmt, _ = pc.case(name)
    for chunk in (1000, 16384):
        assert fc.h_index(H, s, fmt, chunk, lanes=64).key() == fc.h_index(H, s, fmt, chunk).key(), (name, chunk)


# ---- 3. planted streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(fc.PLANTED))
def test_planted_headers_are_dropped(H, truth, name):
    s, fmt, data, planted_bits = fc.planted(name)
    T = truth(s, fmt)
    true_bits = {r[0] for r in T}
    for chunk in fc.PLANTED[name][2]:
        cand = fc.h_candidates(H, s, fmt, chunk)
        for p in planted_bits:                                     # the guards
            assert p in cand, "the planted bit is a candidate"
            assert p not in true_bits, "and no block of the stream starts there"
            assert any(c > p and c in true_bits for c in cand), "a true candidate lies behind it"
        assert T[1][0] not in cand, "the bit behind the stored block is no candidate: the chain breaks there and needs a repair"
        f = fc.h_index(H, s, fmt, chunk)
        assert f.rc == fc.OK and f.out_len == len(data)
        assert not set(planted_bits) & {r[0] for r in f.rows}
        assert {tuple(r) for r in f.rows} <= {tuple(r) for r in T}, "out_byte of every row is the host builder's"
        assert f.rows[0] == [0, 0] and f.rows[-1] == T[-1]
        assert f.dropped >= len(planted_bits) and f.rounds >= 2
        assert f.candidates - f.dropped == len(f.rows) - 1
        # the rows are the candidates on the true chain, all of them
        assert [r[0] for r in f.rows[:-1]] == [c for c in cand if c in true_bits]
        # a limit so small that jobs of the true chain give up and are run again: the same rows
        g = fc.h_index(H, s, fmt, chunk, limit=16)
        assert (g.rc, g.rows, g.out_len, g.dropped) == (f.rc, f.rows, f.out_len, f.dropped)
        assert g.rounds > f.rounds and g.jobs > f.jobs, "jobs of the true chain gave up and were run again"
        assert fc.h_index(H, s, fmt, chunk, lanes=64).key() == f.key()


def test_small_limit_on_clean_streams(H):
    """with a limit of the test's own, 16 bytes behind every start, the jobs of the true chain give up and are run again one by
    one: more rounds, the same rows"""
    for name in ("alice_mem1", "alice_flushes"):
        s, fmt, _ = pc.case(name)
        f, g = fc.h_index(H, s, fmt, 1000), fc.h_index(H, s, fmt, 1000, limit=16)
        assert (g.rc, g.rows, g.out_len, g.candidates, g.dropped) == (f.rc, f.rows, f.out_len, f.candidates, f.dropped)
        assert g.rounds > 1 and g.jobs > f.jobs


# ---- 4. thinning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("alice_l6", "alice_mem1", "alice_flushes", "alice_gzip_header", "mix_mem1"))
def test_thinning(H, name):
    s, fmt, data = pc.case(name)
    chunk = 1000 if name in fc.SMALL else 4096
    full = fc.h_index(H, s, fmt, chunk).rows
    for spacing in (4096, 100000):
        f = fc.h_index(H, s, fmt, chunk, spacing=spacing)
        assert f.rc == fc.OK and f.out_len == len(data)
        assert all(a[1] // spacing < b[1] // spacing for a, b in zip(f.rows[:-1], f.rows[1:-1])), "no two inner rows inside one stretch"
        want, nxt = [], 0                                          # the host builder's rule over the accepted rows
        for bit, pos in full[:-1]:
            if pos >= nxt:
                want.append([bit, pos]); nxt = pos - pos % spacing + spacing
        assert f.rows == want + [full[-1]]


# ---- the edges -------------------------------------------------------------------------------------------------------------------------
def test_header_in_the_last_bits_of_a_chunk(H, truth):
    s, fmt, data = pc.case("alice_mem1")
    d, T = fc.deflate_of(s, fmt), truth(s, fmt)
    starts = fc.dynamic_starts(d, T)
    hits = 0
    for chunk in range(64, 400):
        for p in starts:
            left = -p % (8 * chunk)                                # bits from p to the chunk's end
            c = p // (8 * chunk)
            if not (1 <= left <= 16 and c >= 1) or any(q // (8 * chunk) == c and q < p for q in starts):
                continue
            f = fc.h_index(H, s, fmt, chunk)
            check_against_truth(f, T, s, fmt, chunk, len(data))
            assert p in {r[0] for r in f.rows}, (chunk, p)
            hits += 1
            break
        if hits >= 6:
            break
    assert hits >= 3, "the premise: true headers that start in a chunk's last 1..16 bits"


def test_header_at_a_chunks_first_bit(H, truth):
    s, fmt, data = pc.case("alice_mem1")
    d, T = fc.deflate_of(s, fmt), truth(s, fmt)
    aligned = [p for p in fc.dynamic_starts(d, T) if p % 8 == 0 and p // 8 >= 64]
    assert aligned, "the premise: a byte-aligned block start"
    for p in aligned[:3]:
        chunk = p // 8                                             # chunk 1 begins with the header
        f = fc.h_index(H, s, fmt, chunk)
        check_against_truth(f, T, s, fmt, chunk, len(data))
        assert f.rows[1][0] == p
    # (the planted streams hold one in a later chunk by construction: the guard there asserts that it is a candidate)


@pytest.mark.parametrize("name", fc.SMALL)
def test_stream_shorter_than_one_chunk(H, truth, name):
    s, fmt, data = pc.case(name)
    f = fc.h_index(H, s, fmt, fc.BIGGER_THAN_ANY)
    T = truth(s, fmt)
    assert (f.rc, f.rows, f.out_len) == (fc.OK, [T[0], T[-1]], len(data)) and (f.candidates, f.dropped, f.rounds) == (1, 0, 1)


@pytest.mark.parametrize("name", ("alice_l0", "alice_fixed"))
def test_candidate_free_middle(H, truth, name):
    s, fmt, data = pc.case(name)
    T = truth(s, fmt)
    assert not fc.dynamic_starts(fc.deflate_of(s, fmt), T), "the premise: no non-final dynamic block"
    for chunk in fc.CHUNKS:
        f = fc.h_index(H, s, fmt, chunk)
        assert (f.rc, f.rows, f.out_len) == (fc.OK, [T[0], T[-1]], len(data)), chunk


def test_final_block_alone_in_the_last_chunk(H, truth):
    s, fmt, data = pc.case("alice_l6")
    d, T = fc.deflate_of(s, fmt), truth(s, fmt)
    chunk = 4096
    last_chunk = (len(d) - 1) // chunk
    assert fc.block_type(d, T[-2][0])[0] == 1 and T[-2][0] < 8 * chunk * last_chunk, "the premise: the last chunk lies inside the final block"
    f = fc.h_index(H, s, fmt, chunk)
    check_against_truth(f, T, s, fmt, chunk, len(data))
    assert all(r[0] // (8 * chunk) < last_chunk for r in f.rows[:-1])


def test_header_cut_off_by_the_end_of_the_stream(H):
    """a dynamic header at a chunk's first bit, cut off at every one of its last 40 bytes: the finder reads zeros behind the
    stream and must refuse; with the whole header there it accepts"""
    chunk = 64
    raw = pc.case("alice_raw")[0]
    front = b"\x00" + fc.struct.pack("<HH", chunk - 5, (chunk - 5) ^ 0xFFFF) + bytes(chunk - 5)   # a non-final stored block: D[0, chunk)
    whole = next(n for n in range(1, 400) if fc.h_candidates(H, front + raw[:n], pc.RAW, chunk) == [0, 8 * chunk])
    assert whole > 40, "the premise: a header longer than 40 bytes"
    for n in range(whole - 40, whole):
        s = front + raw[:n]
        assert fc.h_candidates(H, s, pc.RAW, chunk) == [0], n
        assert fc.h_candidates(H, s, pc.RAW, chunk, lanes=64) == [0], n
        assert fc.h_index(H, s, pc.RAW, chunk).rc == fc.DATA, n


# ---- 5. damaged streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.DAMAGED)
def test_damaged_streams(H, truth, name):
    streams, fmt = fc.damaged(name)
    seen = set()
    for s in streams:
        v = pc.zlib_verdict(s, fmt)
        for chunk in (1000, 4096):
            f = fc.h_index(H, s, fmt, chunk)                       # (an abort of the checked build would end the test run)
            assert f.rc in (fc.OK, fc.DATA, fc.UNSUPPORTED), f.rc
            if v is not None:
                check_against_truth(f, truth(s, fmt), s, fmt, chunk, len(v))
            if f.rc == fc.DATA:
                assert v is None, "ZZ_E_DATA only where zlib refuses"
            if f.rc == fc.UNSUPPORTED:
                assert fmt == pc.ZLIB and s[1] & 0x20
            seen.add(f.rc)
    assert fc.DATA in seen and fc.OK in seen, "the list holds streams of both kinds (a wrong checksum alone still gets an index)"


# ---- 6. the stand-alone program under the address sanitizer ----------------------------------------------------------------------------
def test_stand_alone_sanitizer_run(H, tmp_path):
    exe = fc.build_main(tmp_path)
    todo = [(n, pc.case(n)[0], pc.case(n)[1], c) for n in fc.SMALL for c in (64, 1000)]
    todo += [(n, fc.planted(n)[0], fc.planted(n)[1], c) for n in fc.PLANTED for c in fc.PLANTED[n][2]]
    todo += [("flip%d" % i, s, fc.damaged("alice_mem1")[1], 1000) for i, s in enumerate(fc.damaged("alice_mem1")[0][:12])]
    for name, s, fmt, chunk in todo:
        path = os.path.join(str(tmp_path), name + ".bin")
        with open(path, "wb") as fh:
            fh.write(s)
        for limit in (0, 16):
            assert fc.run_main(exe, path, fmt, chunk, 1, limit).key() == fc.h_index(H, s, fmt, chunk, limit=limit).key(), (name, chunk, limit)


def test_zlib_accepts_every_listed_stream():
    for name in fc.CLEAN:
        s, fmt, data = pc.case(name)
        assert zlib.decompress(s, pc.WBITS[fmt]) == data
    for name in fc.PLANTED:
        s, fmt, data, _ = fc.planted(name)
        assert zlib.decompress(s, pc.WBITS[fmt]) == data
