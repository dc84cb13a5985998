"""zz_decode_members_device / Context.decode_members: a file of gzip members back to back -- blocked (BGZF) members in parallel,
anything else serially. The yardstick for every verdict is zlib's own loop over the members (members_cases.yardstick): what it
returns must come back byte for byte, what it refuses must be E_DATA; every case also asserts the path the call reports.
Members are built in Python (raw deflate by zlib, hand-made headers). Needs a real MI355X: run with `-m gpu`."""
import random
import struct

import pytest

import zzflate_amd as zz
import members_cases as mc

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    return zz.Context(0)


def dev(torch, b):
    return torch.frombuffer(bytearray(b) if b else bytearray(1), dtype=torch.uint8).cuda()


def run(torch, ctx, f, cap):
    """(status, decoded bytes, (members, candidates, path)); the guard bytes in front of dst and behind dst[cap) must be untouched"""
    src = dev(torch, f)
    buf = torch.full((cap + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    rc, n = 0, 0
    try:
        n = ctx.decode_members(src.data_ptr(), len(f), buf.data_ptr() + GUARD, cap)
    except zz.ZzFlateError as e:
        rc = e.code
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().tobytes()
    assert raw[:GUARD] == b"\xEE" * GUARD and raw[GUARD + cap:] == b"\xEE" * GUARD, "bytes outside the destination were written"
    return rc, raw[GUARD:GUARD + n], ctx.last_decode_members_stats()


CASES = mc.path_cases()


@pytest.mark.parametrize("name,f,path", CASES, ids=[c[0] for c in CASES])
def test_valid_files_come_back_on_the_expected_path(torch, ctx, name, f, path):
    want = mc.checked(f)
    assert want is not None, "the case is meant to be valid"
    rc, out, (members, cand, p) = run(torch, ctx, f, len(want))
    assert (rc, out) == (0, want)
    assert p == path
    if path == mc.WALKED:
        assert cand > members
    if path == mc.BLOCKED:
        assert cand == members
    rc, out, _ = run(torch, ctx, f, len(want) - 1)
    assert (rc, out) == (zz.E_NOSPACE, b"")


def test_five_thousand_members_of_4_kib(torch, ctx):
    # more members than the 4,096 resident wavefronts, so the dealing counter is used, and candidates in many workgroups
    rng = random.Random(21)
    t = mc.corpus("lcet10.txt") + mc.corpus("alice29.txt")
    ms, parts = [], []
    for k in range(5000):
        at = rng.randrange(len(t) - 4096)
        parts.append(t[at:at + 4096])
        ms.append(mc.bgzf(parts[-1], (1, 6)[k & 1]))
    f, want = b"".join(ms), b"".join(parts)
    assert mc.checked(f) == want
    rc, out, stats = run(torch, ctx, f, len(want))
    assert rc == 0 and out == want
    assert stats == (5000, 5000, mc.BLOCKED)
    assert len(f) > 200 * mc.STRETCH


def test_one_crowded_stretch_among_empty_ones(torch, ctx):
    # the mark pass ranks a stretch's candidates by a scan over its four wavefronts: 120 tiny members fill stretch 16 and its
    # neighbours with headers in every wavefront, between two stored members of 65,280 random bytes whose stretches hold none
    rng = random.Random(33)
    big = [bytes(rng.getrandbits(8) for _ in range(65280)) for _ in range(2)]
    assert all(b"\x1f\x8b\x08" not in b for b in big)
    tiny = [mc.text(20 + k % 13, k) for k in range(120)]
    ms = [mc.bgzf(big[0], 0)] + [mc.bgzf(t) for t in tiny] + [mc.bgzf(big[1], 0), mc.EOF_BLOCK]
    f, want = b"".join(ms), big[0] + b"".join(tiny) + big[1]
    starts = [sum(len(x) for x in ms[:k]) for k in range(len(ms))]
    per_wave = {}
    for s in starts:
        per_wave.setdefault(s // mc.STRETCH, set()).add(s % mc.STRETCH // 1024)
    assert per_wave[16] == {0, 1, 2, 3} and len(per_wave) <= 6 and len(f) > 32 * mc.STRETCH
    assert mc.checked(f) == want
    rc, out, stats = run(torch, ctx, f, len(want))
    assert rc == 0 and out == want
    assert stats == (len(ms), len(ms), mc.BLOCKED)


def test_more_stretches_than_one_round_of_the_scan(torch, ctx):
    # k_members_scan takes 4096 stretches a round: a stored file of a little over 16 MiB, written, read back and compared on the
    # device; the members behind stretch 4095 lie where the first round's count says
    n = (16 << 20) + 3 * zz.MEMBERS_BLOCK + 5
    data = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 9, 0, data, n)
    cap = zz.members_bound(n)
    file = torch.empty(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode_members(data, n, file, cap, level=0)
    members = -(-n // zz.MEMBERS_BLOCK) + 1
    assert w > 4097 * mc.STRETCH and (w - 28 - 2 * zz.MEMBERS_BLOCK) > 4096 * mc.STRETCH      # two members begin in the second round
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert ctx.decode_members(file, w, back, n) == n
    assert torch.equal(back, data)
    assert ctx.last_decode_members_stats() == (members, members, mc.BLOCKED)


def test_member_boundaries_on_every_residue_of_the_stretch(torch, ctx):
    # the second member's header starts at every offset of one stretch of the mark pass and 20 bytes beyond: inside a lane's
    # bytes, across two lanes, across two wavefronts and across two workgroups
    rng = random.Random(4)
    data = bytes(rng.getrandbits(8) for _ in range(8))
    tail_data = mc.text(300, 8)
    tail = mc.bgzf(tail_data) + mc.EOF_BLOCK
    want = torch.frombuffer(bytearray(data + tail_data), dtype=torch.uint8).cuda()
    base = len(mc.bgzf(data, 0, before=mc.subfield(b"ZZ", b"")))
    first = mc.bgzf(data, 0, before=mc.subfield(b"ZZ", b""))
    assert mc.checked(first + tail) == data + tail_data
    buf = torch.empty(len(data + tail_data) + 2 * GUARD, dtype=torch.uint8, device="cuda")
    bad = []
    for size in range(base, base + mc.STRETCH + 20):
        # the filler subfield grows by one byte: XLEN, the filler's SLEN and BSIZE are patched into the header
        k = size - base
        h = bytearray(first[:12]) + b"ZZ" + struct.pack("<H", k) + b"\x00" * k + first[16:]
        h[10:12] = struct.pack("<H", 4 + k + 6)
        h[16 + k + 4:16 + k + 6] = struct.pack("<H", size - 1)
        f = bytes(h) + tail
        if k % 512 == 0:
            assert mc.yardstick(f) == data + tail_data, size
        src = dev(torch, f)
        buf.fill_(0xEE)
        n = ctx.decode_members(src.data_ptr(), len(f), buf.data_ptr() + GUARD, want.numel())
        ok = n == want.numel() and torch.equal(buf[GUARD:GUARD + n], want) and ctx.last_decode_members_stats() == (3, 3, mc.BLOCKED)
        ok = ok and bool((buf[:GUARD] == 0xEE).all()) and bool((buf[GUARD + n:] == 0xEE).all())
        if not ok:
            bad.append(size)
    assert not bad, bad[:20]


REFUSED = mc.refusal_cases()


@pytest.mark.parametrize("name,f", REFUSED, ids=[c[0] for c in REFUSED])
def test_refusals(torch, ctx, name, f):
    assert mc.checked(f) is None, "the case is meant to be refused"
    rc, out, (_, _, p) = run(torch, ctx, f, 40000)
    assert (rc, out) == (zz.E_DATA, b"")
    assert p == (mc.SERIAL if f else 0)                      # a failure is decided by the serial path (an empty file by nobody)


def test_every_truncation_of_a_three_member_file(torch, ctx):
    f, lens = mc.three_members()
    want = mc.checked(f)
    assert 150 <= len(f) <= 260
    assert run(torch, ctx, f, len(want))[:2] == (0, want)
    for k in range(len(f)):
        t = f[:k]
        y = mc.checked(t)
        rc, out, (_, _, p) = run(torch, ctx, t, len(want))
        if y is None:
            assert (rc, out) == (zz.E_DATA, b""), k
            assert p == (mc.SERIAL if k else 0), k           # (an empty file is refused before a path is taken)
        else:                                                # a cut at a member boundary leaves a valid, shorter file
            assert k in (lens[0], lens[0] + lens[1]) and (rc, out) == (0, y), k
            assert p == mc.BLOCKED, k


def test_space(torch, ctx):
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), mc.text(5000, 3)
    f = mc.bgzf(a) + mc.bgzf(b) + mc.bgzf(c)
    n = len(a) + len(b) + len(c)
    rc, out, stats = run(torch, ctx, f, n)                   # cap exact
    assert (rc, out, stats) == (0, a + b + c, (3, 3, mc.BLOCKED))
    for cap in (n - 1, len(a) + 100, len(a), len(a) - 1, 0):  # one short; ending inside the middle member's slot; ...
        rc, out, stats = run(torch, ctx, f, cap)
        assert (rc, out) == (zz.E_NOSPACE, b""), cap
        assert stats[2] == mc.BLOCKED, "a file that is merely too large is refused on the blocked path"
    # only empty members: no room needed
    rc, out, stats = run(torch, ctx, mc.EOF_BLOCK * 3, 0)
    assert (rc, out, stats) == (0, b"", (3, 3, mc.BLOCKED))
    # too large and damaged in a LATER member: the first member in order that fails decides -- no space
    bad_last = bytearray(f); bad_last[-8] ^= 1
    assert mc.checked(bytes(bad_last)) is None
    rc, out, stats = run(torch, ctx, bytes(bad_last), len(a) + 100)
    assert (rc, out, stats[2]) == (zz.E_NOSPACE, b"", mc.BLOCKED)
    rc, out, stats = run(torch, ctx, bytes(bad_last), n)
    assert (rc, out, stats[2]) == (zz.E_DATA, b"", mc.SERIAL)
    # damaged in an EARLIER member: data, however small the room behind it
    bad_first = bytearray(f); bad_first[len(mc.bgzf(a)) - 8] ^= 1
    rc, out, stats = run(torch, ctx, bytes(bad_first), len(a) + 100)
    assert (rc, out, stats[2]) == (zz.E_DATA, b"", mc.SERIAL)
    # a member whose ISIZE lies gets its own slot and no more (run() checks the guards); the serial path decides
    lie = bytearray(f); k = len(mc.bgzf(a))
    for claim, cap in ((len(a) - 10, n), (len(a) + 10, n), (len(a) + 10, len(a) + 5)):
        lie[k - 4:k] = struct.pack("<I", claim)
        assert mc.checked(bytes(lie)) is None
        rc, out, stats = run(torch, ctx, bytes(lie), cap)
        assert (rc, out, stats[2]) == (zz.E_DATA, b"", mc.SERIAL)


def test_a_member_whose_blocks_run_past_its_end(torch, ctx):
    # Cut out by its announced length such a member is followed by zero bits, in the file by the next member's bytes; "no space"
    # from the cut-out member is therefore re-judged by the serial rule from that member on. zlib says where the verdict turns
    # (members_cases.produced); AT the turn the serial rule's own verdict is the recorded one (tests/golden/members_open.json,
    # which tests/test_inflate_members_cpu.py holds to the rule).
    import json
    import os
    rec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "members_open.json")))
    files = list(mc.open_member_files(8))
    assert len(rec) == len(files)
    for (f, front, made), (turn, at_turn) in zip(files, rec):
        assert turn == front + made
        for cap, want in ((turn - 1, zz.E_NOSPACE), (turn, at_turn), (turn + 1, zz.E_DATA)):
            if cap < 0:
                continue
            rc, out, (_, _, p) = run(torch, ctx, f, cap)
            assert (rc, out) == (want, b""), (len(f), cap, turn)
            # (a damaged member's last four bytes are no ISIZE: where they claim little, it is not m*, and the serial path decides)
            assert p == mc.SERIAL or (rc, p) == (zz.E_NOSPACE, mc.BLOCKED), (len(f), cap, p)


def test_argument_errors_with_a_context(torch, ctx):
    import ctypes
    out = ctypes.c_uint64(5)
    src = dev(torch, mc.EOF_BLOCK)
    L = zz.lib
    assert L.zz_decode_members_device(ctx._h, None, 28, None, 0, ctypes.byref(out), None) == zz.E_ARG and out.value == (1 << 64) - 1
    assert L.zz_decode_members_device(ctx._h, src.data_ptr(), 28, None, 0, None, None) == zz.E_ARG
    assert L.zz_decode_members_device(ctx._h, src.data_ptr(), 28, None, 1, ctypes.byref(out), None) == zz.E_ARG
    assert L.zz_decode_members_device(ctx._h, src.data_ptr(), 28, None, 0, ctypes.byref(out), None) == 0 and out.value == 0
    # an unfinished asynchronous encode on the context
    data = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(zz.bound(1000), dtype=torch.uint8, device="cuda")
    ctx.encode_async(data, 1000, dst, dst.numel())
    assert L.zz_decode_members_device(ctx._h, src.data_ptr(), 28, None, 0, ctypes.byref(out), None) == zz.E_ARG
    assert out.value == (1 << 64) - 1
    ctx.finish()


def test_other_last_call_state_is_left_alone(torch, ctx):
    data = mc.corpus("alice29.txt")
    src = dev(torch, data)
    enc = torch.zeros(zz.bound(len(data)), dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, len(data), enc, enc.numel(), zz.Format.Zlib, 2)
    back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    assert ctx.decode(enc, w, back, len(data), zz.Format.Zlib, index=ctx.packet_index()) == len(data)
    before = (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.verify_last())
    assert before[0] == zz.DECODE_INDEXED
    f = mc.bgzf(mc.text(3000, 1)) + mc.member(mc.text(100, 2))
    assert run(torch, ctx, f, 3100)[0] == 0 and run(torch, ctx, mc.EOF_BLOCK, 0)[0] == 0
    assert (ctx.last_decode_path(), ctx.last_decode_stats(), ctx.verify_last()) == before
