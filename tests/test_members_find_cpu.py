"""The members found in parallel, on the CPU: tests/cxx/members_find_harness.cpp restates zz_members_find_device and
zz_decode_members_found_device on the host -- candidates, the measures with their limit, the walk, round 2, the slots, zi_item per
dealt member, zi_members where the procedure says so -- with the rules of zzflate_amd/csrc/zz_inflate_core.h, built with g++
-fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access bounds-checked; out of range aborts), with ONE lane and with 64
simulated lanes. The yardsticks are a pure-Python restatement of the definition (members_find_cases.Expect: candidates by the
header rule, the true chain from zlib's member loop) and zlib's verdict (members_cases.yardstick)."""
import os
import zlib

import pytest

import members_cases as mc
import members_find_cases as fc

VALID = fc.valid_cases()
REFUSED = fc.refusal_cases()
SWEEP = [n for n in REFUSED if n.startswith("three small members cut")]
NAMED = [n for n in REFUSED if n not in SWEEP]
# files small enough for 64 simulated lanes on every run
SMALL = ("one member", "FNAME, FCOMMENT, FHCRC and a non-BC FEXTRA", "BGZF and plain members mixed", "stored bytes that look like headers and like a member",
         "member starts 15, 16 and 17 past a stretch start")


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return fc.build_harness(tmp_path_factory.mktemp("members_find"))


@pytest.fixture(scope="module")
def expect():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = fc.Expect(*VALID[name])
        return memo[name]
    return get


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VALID))
def test_valid_files_equal_the_restatement(H, expect, name):
    f, E = VALID[name][0], expect(name)
    assert fc.h_candidates(H, f) == E.cand
    results = []
    for limit in fc.LIMITS:
        r = fc.h_find(H, f, limit)
        assert (r.rc, r.rows, r.entries) == (fc.OK, E.rows, E.members + 1), limit
        assert (r.members, r.candidates, r.dropped) == (E.members, len(E.cand), E.dropped), limit
        assert r.rounds <= 2 and r.jobs <= 2 * r.candidates
        if E.rounds(limit) is not None:
            assert r.rounds == E.rounds(limit), limit
        results.append(r)
    assert results[0].rounds == 2 or E.members == 1 or max(E.used[1:]) <= 64 + 8, "a limit of 64 bytes makes members give up"
    assert all((r.rc, r.rows, r.members, r.candidates, r.dropped) == (results[0].rc, results[0].rows, results[0].members, results[0].candidates, results[0].dropped)
               for r in results), "the result does not depend on limit_bytes"


def test_the_cases_hold_what_they_are_built_for(expect):
    E = expect("stored bytes that look like headers and like a member")
    f = VALID["stored bytes that look like headers and like a member"][0]
    assert E.dropped >= 2, "the bare magic and the stored member are candidates, and dropped"
    inner = f.find(b"inner\x00") - 10
    assert inner in E.cand and inner not in [r[0] for r in E.rows]
    tail = f.rfind(b"\x1f\x8b\x08\x00\x00\x00")
    assert 0 < len(f) - tail < 20 and tail not in E.cand, "a magic fewer than 20 bytes from the end is no candidate"
    E = expect("ISIZE 1f 8b 08 00 in front of the next member")
    f = VALID["ISIZE 1f 8b 08 00 in front of the next member"][0]
    assert E.rows[1][1] == fc.ISIZE_MAGIC and E.rows[1][0] - 4 in E.cand, "the false header overlaps the true trailer"
    assert E.dropped >= 1
    for at in (fc.STRETCH - 1, fc.STRETCH, fc.STRETCH + 1):
        assert expect(f"a member start at file offset {at}").rows[1][0] == at
    rows = expect("member starts 15, 16 and 17 past a stretch start").rows
    assert [r[0] % fc.STRETCH for r in rows[1:-1:2]] == [fc.PER_LANE - 1, fc.PER_LANE, fc.PER_LANE + 1]
    E = expect("2,000 members of 0..200 bytes")
    assert E.members == 2000 and any(a[1] == b[1] for a, b in zip(E.rows, E.rows[1:])), "empty members among them"
    assert expect("a member many times longer than a small limit").used[1] > 5 * 4096
    for name, (f, _) in VALID.items():
        assert len(f) <= (1 << 20) + 4096, name


@pytest.mark.parametrize("name", SMALL)
def test_sixty_four_lanes(H, name):
    f = VALID[name][0]
    want = mc.checked(f)
    for limit in (64, fc.LIMIT_DEFAULT):
        assert fc.h_find(H, f, limit, lanes=64).key() == fc.h_find(H, f, limit).key()
    assert fc.h_decode(H, f, len(want), lanes=64)[:2] == (fc.OK, want)
    assert fc.h_decode(H, f, len(want) - 1, 64, lanes=64)[:2] == (fc.NOSPACE, None)


def test_the_size_protocol(H, expect):
    f, E = VALID["python gzip.compress members"][0], expect("python gzip.compress members")
    for room in (0, E.members):
        r = fc.h_find(H, f, max_entries=room)
        assert (r.rc, r.entries) == (fc.NOSPACE, E.members + 1)
    assert fc.h_find(H, f, max_entries=E.members + 1).rows == E.rows


# ---- 2. the decode call's verdicts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VALID))
def test_decode_equals_the_yardstick(H, name):
    f = VALID[name][0]
    want = mc.checked(f)
    assert want is not None
    for limit in (64, fc.LIMIT_DEFAULT):
        assert fc.h_decode(H, f, len(want), limit)[:2] == (fc.OK, want), limit
    for cap in (len(want) - 1, 0):                                 # exact above; one short; zero
        rc, out, _ = fc.h_decode(H, f, cap, 4096)
        assert (rc, out) == fc.verdict(want, cap), cap


@pytest.mark.parametrize("name", NAMED)
def test_refusals(H, name):
    f = REFUSED[name]
    room = 40000
    for limit in (64, fc.LIMIT_DEFAULT):
        assert fc.h_decode(H, f, room, limit)[:2] == (fc.DATA, None), limit
    r = fc.h_find(H, f)
    assert r.rc in (fc.OK, fc.DATA) and r.rounds <= 2
    assert fc.h_find(H, f, 64).key()[:3] == r.key()[:3] and fc.h_find(H, f, 4096).key()[:3] == r.key()[:3]
    if "CRC" in name:
        # the CRC is not judged without bytes: the index is the good file's
        assert r.rc == fc.OK and r.members == 3
    elif "blocks" not in name:
        assert r.rc == fc.DATA, "header, ISIZE, padding and the empty file break the walk"


def test_truncation_at_every_byte(H):
    for name in SWEEP:
        f = REFUSED[name]
        assert fc.h_decode(H, f, 200, 64)[:2] == (fc.DATA, None), name
        assert fc.h_find(H, f, 64).rc == fc.DATA, name
        assert fc.h_find(H, f).rc == fc.DATA, name


def test_bad_crc_in_front_of_a_member_that_overflows(H):
    """a bad CRC in member 0 together with a cap that member 2 overflows: members are judged in file order, so E_DATA"""
    f, good, _ = fc.crc_damaged()
    want = mc.checked(good)
    rows, _ = fc.true_chain(good)
    cap = rows[2][1] + 10                                          # members 0 and 1 fit, member 2 does not
    assert fc.h_decode(H, good, cap)[:2] == (fc.NOSPACE, None)
    assert fc.h_decode(H, f, cap)[:2] == (fc.DATA, None)
    assert fc.h_decode(H, f, len(want))[:2] == (fc.DATA, None)
    r = fc.h_find(H, f)
    assert (r.rc, r.rows) == (fc.OK, rows), "the index does not judge checksums"


def test_caps_exact_one_short_and_zero(H):
    f = VALID["FNAME, FCOMMENT, FHCRC and a non-BC FEXTRA"][0]
    want = mc.checked(f)
    rows, _ = fc.true_chain(f)
    for cap in [len(want), len(want) - 1, 0] + [r[1] + d for r in rows[1:-1] for d in (-1, 0, 1)]:
        assert fc.h_decode(H, f, cap, 64)[:2] == fc.verdict(want, cap), cap
    empty = mc.member(b"") + mc.member(b"", 0) + mc.EOF_BLOCK
    assert fc.h_decode(H, empty, 0)[:2] == (fc.OK, b"")


def test_decode_equals_zi_members_on_damaged_members_short_of_room(H, tmp_path_factory):
    """where a member is damaged AND short of room the yardstick needs `produced`: the verdict is zi_members', which
    tests/test_inflate_members_cpu.py holds to zlib -- here the found path must give that verdict too"""
    import ctypes
    import shutil
    import subprocess
    so = os.path.join(str(tmp_path_factory.mktemp("members_truth")), "libinflate_members_harness.so")
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-fPIC", "-shared", "-DZZ_INFLATE_CHECKED", "-o", so,
                    os.path.join(fc.ROOT, "tests", "cxx", "inflate_members_harness.cpp")], check=True)
    T = ctypes.CDLL(so)
    T.zmt_members.restype = ctypes.c_int
    T.zmt_members.argtypes = [ctypes.c_char_p, fc.u64, ctypes.c_void_p, fc.u64, ctypes.c_uint32, ctypes.POINTER(fc.u64), ctypes.POINTER(fc.u64)]
    a, b, c = mc.text(300, 1), mc.text(900, 2), mc.text(500, 3)
    good = mc.member(a) + mc.member(b) + mc.member(c)
    start1 = len(mc.member(a))
    for pos in range(start1 + 12, start1 + len(mc.member(b)), 37):
        f = bytearray(good); f[pos] ^= 0x10
        f = bytes(f)
        for cap in (len(a) + 5, len(a) + 450, len(a) + len(b), len(a) + len(b) + len(c)):
            out = ctypes.create_string_buffer(cap + 1)
            n, m = fc.u64(0), fc.u64(0)
            rc = T.zmt_members(f, len(f), out, cap, 1, ctypes.byref(n), ctypes.byref(m))
            got = fc.h_decode(H, f, cap, 64)
            assert got[0] == rc and (rc != 0 or got[1] == out.raw[:n.value]), (pos, cap)


# ---- 3. the stand-alone program under the address sanitizer ------------------------------------------------------------------------------
def test_stand_alone_sanitizer_run(H, tmp_path):
    exe = fc.build_main(tmp_path)
    todo = [(n, VALID[n][0]) for n in SMALL] + [(n, REFUSED[n]) for n in NAMED] + [(n, REFUSED[n]) for n in SWEEP[::7]]
    for k, (name, f) in enumerate(todo):
        path = os.path.join(str(tmp_path), "case%d.bin" % k)
        with open(path, "wb") as fh:
            fh.write(f)
        want = mc.yardstick(f)
        cap = len(want) if want is not None else 40000
        for limit in (64, fc.LIMIT_DEFAULT):
            found, dec = fc.run_main(exe, path, limit, cap)
            assert found.key() == fc.h_find(H, f, limit).key(), (name, limit)
            rc, out, _ = fc.h_decode(H, f, cap, limit)
            assert dec == ((rc, len(out), zlib.crc32(out)) if rc == fc.OK else (rc, 0, 0)), (name, limit)
