"""The rules of zz_decode_members_ranges_device (zzflate_amd/csrc/zz_inflate_core.h, zi_mr_*) on the CPU, before a kernel runs:
tests/cxx/inflate_members_ranges_harness.cpp restates the device's procedure with the functions the kernels call and zi_item,
built with -DZZ_INFLATE_CHECKED -Wall -Wextra -Werror and no sanitizer flag -- the checked views are the bounds check, and an
access out of range aborts the process. It is held to the yardstick (members_ranges_cases.Judge: zlib's verdict on every member
the index cuts out) on the whole case list, damaged files and lying indexes included, with the product's stage and with a stage
of 700 bytes, where a file of 30,000 bytes takes dozens of waves and most members of the other files are too big to stage. The
guards prove by computation that the list holds the reads it is meant to hold; members_index_from_offsets is checked here too."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import zzflate_amd as zz
import members_cases as mc
import members_ranges_cases as rc

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_members_ranges_harness.cpp")
u64 = ctypes.c_uint64
SMALL_STAGE = 700


def build(tmp, name, *defines):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the members-ranges harness")
    so = str(tmp / name)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-DZZ_INFLATE_CHECKED", *defines,
                    "-o", so, HARNESS], check=True)
    L = ctypes.CDLL(so)
    L.zmr_stage.restype = u64
    L.zmr_reads.restype = ctypes.c_int
    L.zmr_reads.argtypes = [ctypes.c_char_p, u64, ctypes.c_void_p, u64, u64] + [ctypes.c_void_p] * 6 + [ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32)]
    return L


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("members_ranges")
    big, small = build(tmp, "libmr.so"), build(tmp, "libmr_small.so", f"-DZZ_MR_STAGE={SMALL_STAGE}ull")
    assert big.zmr_stage() == rc.STAGE and small.zmr_stage() == SMALL_STAGE
    return {rc.STAGE: big, SMALL_STAGE: small}


def run(H, file, idx, reads):
    """(return code, [(status, bytes or None)], members decoded, waves) of the harness; guard bytes and, for failed reads, the
    bytes behind cap must come back untouched"""
    k = len(reads)
    offs, caps, size = rc.layout(reads, idx)
    raw = ctypes.create_string_buffer(b"\xEE" * (size + 16), size + 16)
    base = (-ctypes.addressof(raw)) % 16                          # the buffer's residue is 0
    words = (u64 * (2 * len(idx)))(*[v % rc.U64 for p in idx for v in p])
    firsts = (u64 * k)(*[r[0] for r in reads])
    nbytes = (u64 * k)(*[r[1] for r in reads])
    dsts = (u64 * k)(*[ctypes.addressof(raw) + base + o for o in offs])
    cps = (u64 * k)(*caps)
    lens = (u64 * k)(*([7] * k))
    status = (ctypes.c_int32 * k)(*([7] * k))
    dec, waves = u64(99), ctypes.c_uint32(99)
    code = H.zmr_reads(file, len(file), words, len(idx), k, firsts, nbytes, dsts, cps, lens, status, ctypes.byref(dec), ctypes.byref(waves))
    img = raw.raw[base:]
    res, used = [], bytearray(len(img))
    for r in range(k):
        o, cp = offs[r], caps[r]
        if status[r] == 0:
            assert lens[r] <= cp, (r, reads[r])
            res.append((0, img[o:o + lens[r]]))
            used[o:o + lens[r]] = b"\x01" * lens[r]
        else:
            assert lens[r] == rc.U64 - 1, (r, reads[r])
            res.append((status[r], None))
            used[o:o + cp] = b"\x01" * cp                         # unspecified inside cap, untouched behind it
    stray = [i for i in range(len(img)) if not used[i] and img[i] != 0xEE]
    assert not stray, ("bytes outside the destinations were written", stray[:8])
    return code, res, dec.value, waves.value


CASES = rc.all_cases()


@pytest.mark.parametrize("stage", [rc.STAGE, SMALL_STAGE])
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_harness_meets_the_yardstick(harnesses, case, stage):
    name, file, idx, reads = CASES[case]
    J = rc.Judge(file, idx, stage)
    want_code, want = J.call(reads)
    code, got, dec, waves = run(harnesses[stage], file, idx, reads)
    for r, (w, g) in enumerate(zip(want, got)):
        assert w == g, (name, r, reads[r], w[0], g[0])
    assert code == want_code
    assert dec == J.decoded(reads)
    if stage == rc.STAGE:
        assert waves == (1 if dec else 0)
    elif name == "300 members of 100 bytes":
        assert waves >= 30000 // (SMALL_STAGE + 100)


def test_one_read_per_call_gives_the_same_answers(harnesses):
    name, file, idx, reads = CASES[1]
    J = rc.Judge(file, idx)
    for r in reads[::7]:
        code, got, _, _ = run(harnesses[rc.STAGE], file, idx, [r])
        assert got[0] == J.read(*r) and code == got[0][0], (r,)


def test_good_files_are_read_as_zlibs_member_loop_reads_them():
    for name, file, idx in rc.good_files():
        whole = mc.checked(file[:idx[-1][0]])
        assert whole is not None and len(whole) == idx[-1][1], name
        J = rc.Judge(file, idx)
        for first, nbytes, cap in rc.reads_for(idx):
            st, m, cp = rc.plan(idx, first, nbytes, cap)
            assert J.read(first, nbytes, cap) == ((st, whole[first:first + m]) if st == 0 else (st, None)), (name, first, nbytes, cap)


def test_damaged_files_fail_only_where_zlib_refuses_a_member():
    for name, file, idx in rc.damaged_files():
        assert mc.yardstick(file) is None, name                  # the file as a whole is refused
        J = rc.Judge(file, idx)
        bad = [j for j in range(len(idx) - 1) if J.member(j) is None]
        assert bad == [1], (name, bad)
        sts = [J.read(*r)[0] for r in rc.reads_for(idx)]
        assert rc.E_DATA in sts and rc.OK in sts, name


def touched(idx, first, m):
    u = [p[1] for p in idx]
    return [j for j in range(len(u) - 1) if u[j + 1] > u[j] and u[j] < first + m and u[j + 1] > first]


def test_the_list_holds_the_reads_it_is_meant_to_hold():
    three = skips = behind_two = False
    residues = set()
    for name, file, idx, reads in CASES:
        if not rc.index_ok(file, idx):
            continue
        u = [p[1] for p in idx]
        offs, _, _ = rc.layout(reads, idx)
        residues |= {o % 16 for o in offs}
        for first, nbytes, cap in reads:
            st, m, _ = rc.plan(idx, first, nbytes, cap)
            if st or not m:
                continue
            t = touched(idx, first, m)
            three |= len(t) >= 3
            empties = [j for j in range(len(u) - 1) if u[j] == first and u[j + 1] == first]
            skips |= bool(empties) and min(empties) < t[0]
            behind_two |= len([j for j in empties if j < t[0]]) >= 2 and u[t[0]] == first and first > 0
    assert three, "no read touches three members"
    assert skips, "no read skips an empty member at its first byte"
    assert behind_two, "no read begins on the first byte behind two empty members"
    assert residues == set(range(16)), residues


def test_members_index_from_offsets():
    def by_lengths(member_lens, n, block, eof):
        idx, c = [], 0
        for i, ln in enumerate(member_lens):
            idx.append((c, min(i * block, n)))
            c += ln
        idx.append((c, n))
        if eof:
            idx.append((c + 28, n))
        return idx
    for n, block in ((0, 100), (1, 100), (250, 100), (300, 100), (65280 * 2, 65280), (65280 * 2 + 1, 65280)):
        members = -(-n // block)
        lens = [40 + 3 * i for i in range(members)]
        offsets = [sum(lens[:i]) for i in range(members + 1)]
        for eof in (True, False):
            got = zz.members_index_from_offsets(offsets, n, block_size=block, eof=eof)
            assert got == by_lengths(lens, n, block, eof), (n, block, eof)
            assert got[-1][1] == n and len(got) == members + 1 + (1 if eof else 0)
    with pytest.raises(ValueError):
        zz.members_index_from_offsets([0, 10], 250, block_size=100)
    # a real blocked file: what the writer's offsets would be for members of 100 input bytes
    name, file, idx = rc.good_files()[3]
    assert zz.members_index_from_offsets([p[0] for p in idx[:-1]], 30000, block_size=100, eof=True) == idx
