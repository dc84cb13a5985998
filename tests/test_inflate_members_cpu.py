"""The member-file rules (zzflate_amd/csrc/zz_inflate_core.h) on the CPU, before a kernel runs: zi_members -- the routine
k_inflate_members runs and the definition of zz_decode_members_device's result -- with ONE lane and with 64 simulated lanes,
zi_bc_len, and a host restatement of the blocked path (candidates, chain check, hop, slots, zi_item per dealt member, verdict)
with the functions the kernels call. tests/cxx/inflate_members_harness.cpp is built with g++ -fsanitize=undefined
-DZZ_INFLATE_CHECKED, so every buffer access of the core is bounds-checked. The yardstick for every verdict is zlib's own loop
over the members (members_cases.yardstick): what it returns must come back byte for byte, what it refuses must be E_DATA."""
import ctypes
import json
import os
import random
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT

import zzflate_amd as zz
import members_cases as mc

HARNESS = os.path.join(ROOT, "tests", "cxx", "inflate_members_harness.cpp")
u64 = ctypes.c_uint64
GUARD = 64
LANES = (1, 64)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the members harness")
    so = str(tmp_path_factory.mktemp("members") / "libinflate_members_harness.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-DZZ_INFLATE_CHECKED", "-o", so, HARNESS],
                   check=True)
    L = ctypes.CDLL(so)
    L.zmt_members.restype = ctypes.c_int
    L.zmt_members.argtypes = [ctypes.c_char_p, u64, ctypes.c_void_p, u64, ctypes.c_uint32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.zmt_bc_len.restype = ctypes.c_uint32
    L.zmt_bc_len.argtypes = [ctypes.c_char_p, u64]
    L.zmt_blocked.restype = ctypes.c_int
    L.zmt_blocked.argtypes = [ctypes.c_char_p, u64, ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64),
                              ctypes.POINTER(ctypes.c_int)]
    return L


def serial(H, f, cap, lanes):
    """(status, bytes, members) of zi_members; the guard bytes around the destination must come back untouched"""
    buf = ctypes.create_string_buffer(b"\xEE" * (cap + 2 * GUARD), cap + 2 * GUARD)
    n, m = u64(0), u64(0)
    rc = H.zmt_members(f, len(f), ctypes.addressof(buf) + GUARD, cap, lanes, ctypes.byref(n), ctypes.byref(m))
    assert rc != -100, "the simulated lanes disagree"
    assert buf.raw[:GUARD] == b"\xEE" * GUARD and buf.raw[GUARD + cap:] == b"\xEE" * GUARD, "bytes outside the destination were written"
    assert rc == 0 or n.value == 0
    return rc, buf.raw[GUARD:GUARD + n.value], m.value


def blocked(H, f, cap):
    """(status, bytes, members, candidates, path) of the host restatement of the device's procedure"""
    buf = ctypes.create_string_buffer(b"\xEE" * (cap + 2 * GUARD), cap + 2 * GUARD)
    n, m, cand, path = u64(0), u64(0), u64(0), ctypes.c_int(0)
    rc = H.zmt_blocked(f, len(f), ctypes.addressof(buf) + GUARD, cap, ctypes.byref(n), ctypes.byref(m), ctypes.byref(cand), ctypes.byref(path))
    assert rc != -100
    assert buf.raw[:GUARD] == b"\xEE" * GUARD and buf.raw[GUARD + cap:] == b"\xEE" * GUARD, "bytes outside the destination were written"
    return rc, buf.raw[GUARD:GUARD + n.value], m.value, cand.value, path.value


def verdict(H, f, cap):
    """the one verdict every path gives for (file, cap): (status, bytes); asserts they agree"""
    got = blocked(H, f, cap)
    for lanes in LANES:
        s = serial(H, f, cap, lanes)
        assert s[:2] == got[:2], ("the blocked procedure and the serial rule disagree", lanes, s[0], got[0], got[4])
    return got


def test_bc_len(H):
    def bc(h):
        return H.zmt_bc_len(h, len(h))
    m = mc.bgzf(b"hello")
    assert bc(m) == len(m) and bc(m + b"tail") == len(m)
    assert bc(mc.EOF_BLOCK) == 28
    for k in range(len(m)):                                  # a header cut short announces nothing -- or, whole, its length
        assert bc(m[:k]) == (len(m) if k >= 18 else 0), k
    # other subfields in front of BC, a BC of another length in front of the one that counts, a second BC behind it
    x = mc.bgzf(b"hello", before=mc.subfield(b"AB", b"xyz") + mc.subfield(b"BC", b"123") + mc.subfield(b"CB", b""), after=mc.subfield(b"BC", b"\x01\x00"))
    assert bc(x) == len(x)
    # not at htslib's offset 12, and nothing announced without FEXTRA, with a reserved flag bit, with another method or magic
    assert x[12:14] != b"BC"
    for pos, val in ((0, 0x1e), (1, 0x8a), (2, 7), (3, 0), (3, 0x24), (3, 0x44), (3, 0x84)):
        b = bytearray(m); b[pos] = val
        assert bc(bytes(b)) == 0, (pos, val)
    for flg in (4, 6, 12, 20, 30):
        b = bytearray(m); b[3] = flg
        assert bc(bytes(b)) == len(m)
    # XLEN that passes the bytes given; a subfield that runs past XLEN; stray bytes that are no subfield; no BC at all
    b = bytearray(m); b[10:12] = struct.pack("<H", len(m) - 12 + 1)
    assert bc(bytes(b)) == 0
    h = b"\x1f\x8b\x08\x04" + b"\x00" * 6
    def with_extra(e, claim=None):
        return h + struct.pack("<H", len(e) if claim is None else claim) + e + b"\x03\x00" + b"\x00" * 8
    assert bc(with_extra(b"BC\x02\x00\x1b\x00")) == 28
    assert bc(with_extra(b"AB\x09\x00xyBC\x02\x00\x1b\x00")) == 0            # AB runs past XLEN
    assert bc(with_extra(b"BC\x02\x00\x1b")) == 0                            # BC's payload cut by XLEN
    assert bc(with_extra(b"BC\x02\x00\x1b\x00", claim=5)) == 0
    assert bc(with_extra(b"AB\x01\x00xBC\x02")) == 0
    assert bc(with_extra(b"")) == 0 and bc(with_extra(b"AB\x00\x00")) == 0
    # a length that cannot hold the header, two bytes of blocks and the trailer
    assert bc(with_extra(b"BC\x02\x00\x1a\x00")) == 0 and bc(with_extra(b"BC\x02\x00\x00\x00")) == 0
    assert bc(with_extra(b"ZZ\x04\x00abcdBC\x02\x00\x22\x00")) == 0 and bc(with_extra(b"ZZ\x04\x00abcdBC\x02\x00\x23\x00")) == 36
    assert bc(with_extra(b"BC\x02\x00\xff\xff")) == 65536


CASES = mc.path_cases()


@pytest.mark.parametrize("name,f,path", CASES, ids=[c[0] for c in CASES])
def test_valid_files_come_back_on_the_expected_path(H, name, f, path):
    want = mc.checked(f)
    assert want is not None, "the case is meant to be valid"
    rc, out, members, cand, p = verdict(H, f, len(want))
    assert (rc, out) == (0, want)
    assert p == path
    if path == mc.WALKED:
        assert cand > members
    if path == mc.BLOCKED:
        assert cand == members
    # room to spare changes nothing; one byte short is E_NOSPACE on every path (an empty file of members needs no room)
    assert verdict(H, f, len(want) + 100)[:2] == (0, want)
    if want:
        assert verdict(H, f, len(want) - 1)[:2] == (zz.E_NOSPACE, b"")


REFUSED = mc.refusal_cases()


@pytest.mark.parametrize("name,f", REFUSED, ids=[c[0] for c in REFUSED])
def test_refusals(H, name, f):
    assert mc.checked(f) is None, "the case is meant to be refused"
    rc, out, _, _, p = verdict(H, f, 40000)
    assert (rc, out) == (zz.E_DATA, b"")
    assert p in (0, mc.SERIAL)                               # a failure is decided by the serial rule (an empty file by nobody)


def test_every_truncation_of_a_three_member_file(H):
    f, lens = mc.three_members()
    want = mc.checked(f)
    assert 150 <= len(f) <= 260 and verdict(H, f, len(want))[:2] == (0, want)
    for k in range(len(f)):
        t = f[:k]
        y = mc.checked(t)
        rc, out, _, _, p = verdict(H, t, len(want))
        if y is None:
            assert (rc, out) == (zz.E_DATA, b""), k
            assert p == (mc.SERIAL if k else 0), k           # (an empty file is refused before a path is taken)
        else:                                                # a cut at a member boundary leaves a valid, shorter file
            assert k in (lens[0], lens[0] + lens[1]) and (rc, out) == (0, y), k
            assert p == mc.BLOCKED, k


def test_a_flipped_bit_at_every_byte_agrees_with_zlib(H):
    f, _ = mc.three_members()
    want = mc.checked(f)
    for i in range(len(f)):
        for bit in (0, 5):
            b = bytearray(f); b[i] ^= 1 << bit
            t = bytes(b)
            y = mc.checked(t)
            rc, out = verdict(H, t, len(want) + 300)[:2]
            if y is None:
                assert rc in (zz.E_DATA, zz.E_NOSPACE) and out == b"", (i, bit)    # (a damaged length can ask for more room first)
            else:
                assert (rc, out) == (0, y), (i, bit)


def test_space(H):
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), mc.text(5000, 3)
    f = mc.bgzf(a) + mc.bgzf(b) + mc.bgzf(c)
    n = len(a) + len(b) + len(c)
    assert verdict(H, f, n)[:2] == (0, a + b + c)
    assert verdict(H, f, n)[4] == mc.BLOCKED
    for cap in (n - 1, len(a) + 100, len(a), len(a) - 1, 0):
        got = verdict(H, f, cap)
        assert got[:2] == (zz.E_NOSPACE, b""), cap
        assert got[4] == mc.BLOCKED, "a file that is merely too large is refused on the blocked path"
    # only empty members: no room needed
    assert verdict(H, mc.EOF_BLOCK * 3, 0)[:2] == (0, b"")
    # too large and damaged in a LATER member: the first member in order that fails decides -- no space
    bad_last = bytearray(f); bad_last[-8] ^= 1
    got = verdict(H, bytes(bad_last), len(a) + 100)
    assert got[:2] + got[4:] == (zz.E_NOSPACE, b"", mc.BLOCKED)
    got = verdict(H, bytes(bad_last), n)
    assert got[:2] + got[4:] == (zz.E_DATA, b"", mc.SERIAL)
    # damaged in an EARLIER member: data, however small the room behind it
    bad_first = bytearray(f); bad_first[len(mc.bgzf(a)) - 8] ^= 1
    got = verdict(H, bytes(bad_first), len(a) + 100)
    assert got[:2] + got[4:] == (zz.E_DATA, b"", mc.SERIAL)
    # a member whose ISIZE lies cannot write into its neighbour's slot: the verdict is the serial rule's
    lie = bytearray(f); k = len(mc.bgzf(a))
    for claim, cap in ((len(a) - 10, n), (len(a) + 10, n), (len(a) + 10, len(a) + 5)):
        lie[k - 4:k] = struct.pack("<I", claim)
        got = verdict(H, bytes(lie), cap)
        assert got[:2] + got[4:] == (zz.E_DATA, b"", mc.SERIAL), (claim, cap)


def test_a_member_whose_blocks_run_past_its_end_at_every_cap(H):
    # Cut out by its announced length, such a member is followed by nothing, and a decoder reads zero bits behind it; in the file
    # it is followed by the next member's bytes. What the two readings make of those bits may differ -- a literal that asks for
    # room on one side, an end of block, a far distance or no code on the other -- so "no space" from the cut-out member is not
    # yet the file's verdict. The procedure is held to the serial rule (one lane; the lanes' agreement is the other tests') at
    # the caps around the bytes the damaged member produces, for many places its blocks can be cut and several followers.
    # zlib says where the verdict turns (members_cases.produced): the caps around that place are the ones that matter.
    turned = 0
    for f, front, made in mc.open_member_files(2):
        assert mc.yardstick(f) is None
        for cap in range(max(front + made - 3, 0), front + made + 3):
            got, want = blocked(H, f, cap), serial(H, f, cap, 1)
            assert got[:2] == want[:2], ("the blocked procedure and the serial rule disagree", len(f), cap, got[0], want[0])
            if cap != front + made:                          # (at the turn itself zlib and the serial rule may order the two differently)
                assert got[:2] == ((zz.E_NOSPACE if cap < front + made else zz.E_DATA), b""), (len(f), cap, front, made)
            assert got[0] in (zz.E_NOSPACE, zz.E_DATA) and got[1] == b""
            # (a damaged member's last four bytes are no ISIZE: where they claim little, it is not m*, and the serial rule decides)
            assert got[4] == mc.SERIAL or (got[0], got[4]) == (zz.E_NOSPACE, mc.BLOCKED)
        turned += made > 0
    assert turned > 100, "the sweep does not reach the case it is for"


def test_recorded_verdicts_at_the_turn_are_the_serial_rule_s(H):
    # tests/golden/members_open.json holds, for every 8th cut, the serial rule's verdict at the cap where it turns: the GPU test
    # holds the device to it, this one holds the record to the rule
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "members_open.json")))
    files = list(mc.open_member_files(8))
    assert len(rec) == len(files) and {v for _, v in rec} == {zz.E_NOSPACE, zz.E_DATA}
    for (f, front, made), (cap, want) in zip(files, rec):
        assert cap == front + made
        for lanes in LANES:
            assert serial(H, f, cap, lanes)[:2] == (want, b"")
        assert blocked(H, f, cap)[:2] == (want, b"")


def test_boundaries_on_many_residues_and_random_chains(H):
    rng = random.Random(9)
    tail = mc.bgzf(mc.text(200, 6))
    for size in list(range(mc.BGZF_MIN, mc.BGZF_MIN + 40)) + [rng.randrange(mc.BGZF_MIN, 5000) for _ in range(40)]:
        f = mc.bgzf_sized(size, rng) + tail + mc.EOF_BLOCK
        want = mc.checked(f)
        rc, out, members, cand, p = verdict(H, f, len(want))
        assert (rc, out, members, cand, p) == (0, want, 3, 3, mc.BLOCKED), size
    for _ in range(30):
        ms = []
        for _ in range(rng.randrange(1, 8)):
            kind = rng.randrange(4)
            data = mc.text(rng.randrange(0, 3000), rng.randrange(100))
            ms.append(mc.bgzf(data, rng.choice((0, 1, 6, 9))) if kind else mc.member(data))
        f = b"".join(ms)
        want = mc.checked(f)
        assert verdict(H, f, len(want))[:2] == (0, want)


def test_random_bytes_end_with_a_status(H):
    rng = random.Random(12)
    head = mc.bgzf(b"a member in front")
    for k in range(600):
        s = bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 300)))
        for f in (s, head + s, head + b"\x1f\x8b\x08\x04" + s):
            rc, out = verdict(H, f, 4096)[:2]
            y = mc.yardstick(f)
            if y is not None and len(y) <= 4096:
                assert (rc, out) == (0, y)
            else:
                assert rc in (zz.E_DATA, zz.E_NOSPACE)
