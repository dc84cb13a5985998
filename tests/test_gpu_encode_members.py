"""zz_encode_members_device / Context.encode_members: one buffer to one blocked gzip (BGZF) file. The file, its length, the
offsets array and the statistics equal what the format rule composes from the oracle (members_write_cases.expected), for every
level and the whole case list; the files decode on the device (in parallel where nothing in the input looks like a header) and
with gzip.decompress; pieces concatenate; a file that does not fit leaves the destination untouched. Needs a real MI355X: run
with `-m gpu`."""
import ctypes
import gzip

import pytest

import zzflate_amd as zz
import members_cases as mc
import members_write_cases as mw

pytestmark = pytest.mark.gpu
SLACK = 96
ERR = (1 << 64) - 1


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


def write(torch, ctx, data, level, B, P, eof, cap=None, src=None):
    """(file, bytes behind it up to the end of the allocation, offsets, stats): the destination has `cap` bytes (default: the
    bound) and SLACK bytes of zeros behind them"""
    src = dev(torch, data) if src is None else src
    cap = zz.members_bound(len(data), B, P, eof) if cap is None else cap
    dst = torch.zeros(cap + SLACK, dtype=torch.uint8, device="cuda")
    members = -(-len(data) // B)
    offs = torch.full((members + 1,), -1, dtype=torch.int64, device="cuda")
    w = ctx.encode_members(src, len(data), dst, cap, level, B, P, eof, offs)
    torch.cuda.synchronize()
    raw = dst.cpu().numpy().tobytes()
    return raw[:w], raw[w:], offs.cpu().tolist(), ctx.last_encode_members_stats()


def decoded(torch, ctx, file, n):
    out = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    w = ctx.decode_members(dev(torch, file), len(file), out, n + 1)
    return out[:w].cpu().numpy().tobytes(), ctx.last_decode_members_stats()[2]


@pytest.mark.parametrize("level", mw.LEVELS)
def test_byte_for_byte_and_round_trip(torch, ctx, oracle, level):
    for index, (name, data, B, P, eof) in enumerate(mw.cases(oracle)):
        want, offsets, stored = mw.expected_case(oracle, index, level)
        file, behind, offs, stats = write(torch, ctx, data, level, B, P, eof)
        assert file == want, (name, len(file), len(want))
        assert behind == bytes(len(behind)), name                              # nothing written behind the file
        assert offs == offsets, name
        assert stats == (len(stored), sum(stored)), name
        if file:
            back, path = decoded(torch, ctx, file, len(data))
            assert back == data, name
            if b"\x1f\x8b\x08" not in data:
                assert path == zz.MEMBERS_BLOCKED, name
            assert gzip.decompress(file) == data, name


def test_a_blocked_file_inside_a_blocked_file(torch, ctx, oracle):
    inner, _, _ = mw.expected(oracle, mw.text(20000, 3), 0, 4096, 4096, True)         # stored: its headers stand in the input as they are
    want, _, stored = mw.expected(oracle, inner, 0, 8192, 4096, True)
    file, behind, _, stats = write(torch, ctx, inner, 0, 8192, 4096, True)
    assert file == want and behind == bytes(len(behind)) and stats == (len(stored), 0)
    back, path = decoded(torch, ctx, file, len(inner))
    assert back == inner and path in (zz.MEMBERS_BLOCKED, zz.MEMBERS_WALKED)
    assert mc.yardstick(back) == mw.text(20000, 3)


@pytest.mark.parametrize("level", [0, 1])
def test_more_members_than_one_round_of_the_size_scan(torch, ctx, oracle, level):
    # k_mw_sizes places 4096 members a round: 4097 members of the smallest block there is, one byte, so that the last member and
    # the file's end lie where the first round's bytes say (a member of one byte has 32 bytes stored and 29 compressed)
    B, P = 1, mw.PACKET
    data = mw.text(4097, 11)
    want, offsets, stored = mw.expected(oracle, data, level, B, P, True)
    assert offsets == [(29 if level else 32) * i for i in range(4098)]
    file, behind, offs, stats = write(torch, ctx, data, level, B, P, True)
    assert file == want and behind == bytes(len(behind))
    assert offs == offsets
    assert stats == (4097, sum(stored))
    assert decoded(torch, ctx, file, len(data)) == (data, zz.MEMBERS_BLOCKED)
    assert gzip.decompress(file) == data


@pytest.mark.parametrize("level", [1, 2])
def test_pieces_concatenate(torch, ctx, oracle, level):
    B, P = 4096, 4096
    data = mw.mixed(30000, 30000, 30000, 12)
    cuts = [0, 5 * B, 12 * B, len(data)]                                              # pieces of whole blocks, the last one not
    pieces = [write(torch, ctx, data[a:b], level, B, P, k == 2)[0] for k, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    joined = b"".join(pieces)
    assert joined == mw.expected(oracle, data, level, B, P, True)[0]                   # the members of the one-call file
    assert joined == write(torch, ctx, data, level, B, P, True)[0]
    assert decoded(torch, ctx, joined, len(data))[0] == data
    assert gzip.decompress(joined) == data


@pytest.mark.parametrize("eof", [True, False])
def test_room(torch, ctx, oracle, eof):
    data = mw.mixed(40000, 100000, 60000, 2)
    for level in (0, 1):
        want = mw.expected(oracle, data, level, mw.BLOCK, mw.PACKET, eof)[0]
        file, behind, _, _ = write(torch, ctx, data, level, mw.BLOCK, mw.PACKET, eof, cap=len(want))
        assert file == want and behind == bytes(SLACK)
        src = dev(torch, data)
        cap = len(want) - 1
        dst = torch.full((cap + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
        out = ctypes.c_uint64(0)
        rc = zz.lib.zz_encode_members_device(ctx._h, src.data_ptr(), len(data), dst.data_ptr(), cap, ctypes.byref(out), level, 0, 0,
                                             0 if eof else zz.MEMBERS_NO_EOF, None, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (rc, out.value) == (zz.E_NOSPACE, ERR)
        assert dst.cpu().numpy().tobytes() == b"\xa5" * (cap + SLACK)                 # an untouched destination
        assert ctx.last_encode_members_stats() == (0, 0)


def test_an_empty_input(torch, ctx):
    assert write(torch, ctx, b"", 1, mw.BLOCK, mw.PACKET, True)[0] == mc.EOF_BLOCK
    file, behind, offs, stats = write(torch, ctx, b"", 1, mw.BLOCK, mw.PACKET, False)
    assert (file, offs, stats) == (b"", [0], (0, 0)) and behind == bytes(SLACK)
    with pytest.raises(zz.ZzFlateError) as e:
        write(torch, ctx, b"", 1, mw.BLOCK, mw.PACKET, True, cap=27)
    assert e.value.code == zz.E_NOSPACE


def test_refusals_before_launch(torch, oracle):
    data = mw.text(70000, 4)
    src = dev(torch, data)
    dst = torch.zeros(80000, dtype=torch.uint8, device="cuda")
    c = zz.Context(0)

    def code(*a, **k):
        with pytest.raises(zz.ZzFlateError) as e:
            c.encode_members(src, len(data), dst, 80000, *a, **k)
        assert c.last_encode_members_stats() == (0, 0)
        return e.value.code
    assert code(1, 65280, 1000) == zz.E_ARG
    assert code(1, 65537) == zz.E_ARG
    assert code(1, 65280, 32769) == zz.E_ARG
    assert code(4) == -1
    assert code(-1) == -1
    assert code(1, offsets=torch.zeros(2, dtype=torch.int64, device="cuda")) == zz.E_ARG          # two members: three offsets
    c.set_warm_window(4096)
    assert code(1) == zz.E_UNSUPPORTED
    c.set_warm_window(0)
    assert c.encode_members(src, len(data), dst, 80000, 1) == len(mw.expected(oracle, data, 1, mw.BLOCK, mw.PACKET, True)[0])
    assert c.last_encode_members_stats() == (2, 0)
    c.set_extended_levels(True)
    assert code(1) == zz.E_UNSUPPORTED
    assert code(6) == zz.E_UNSUPPORTED
    c.set_extended_levels(False)
    out = ctypes.c_uint64(0)
    dst.zero_()
    assert zz.lib.zz_encode_members_device(c._h, None, 5, dst.data_ptr(), 80000, ctypes.byref(out), 1, 0, 0, 0, None, 0, None) == zz.E_ARG
    assert out.value == ERR
    assert zz.lib.zz_encode_members_device(c._h, src.data_ptr(), 5, dst.data_ptr(), 80000, None, 1, 0, 0, 0, None, 0, None) == zz.E_ARG
    assert zz.lib.zz_encode_members_device(c._h, src.data_ptr(), 5, None, 80000, ctypes.byref(out), 1, 0, 0, 0, None, 0, None) == zz.E_ARG
    torch.cuda.synchronize()
    assert dst.count_nonzero().item() == 0                                     # none of the refused calls wrote a byte
    c.close()


@pytest.mark.parametrize("level", [1, 2])
def test_lds_order_rerun_writes_the_same_bytes(torch, ctx, oracle, level):
    data = mw.mixed(40000, 100000, 60000, 2)
    want, offsets, stored = mw.expected(oracle, data, level, mw.BLOCK, 4096, True)
    try:
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_violation(1)             # the kernel reports a violation: the whole call runs again
        file, behind, offs, stats = write(torch, ctx, data, level, mw.BLOCK, 4096, True)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 0
        assert file == want and behind == bytes(len(behind)) and offs == offsets and stats == (len(stored), sum(stored))
        # and on the one-parser forms from the start
        assert write(torch, ctx, data, level, mw.BLOCK, 4096, True)[0] == want
    finally:
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


@pytest.mark.parametrize("level", mw.LEVELS)
def test_a_source_at_an_odd_offset(torch, ctx, oracle, level):
    data = mw.mixed(40000, 100000, 60000, 2)
    big = dev(torch, b"\x55" * 4097 + data + b"\xaa" * 100)
    want = mw.expected(oracle, data, level, 8192, 4096, True)[0]
    assert write(torch, ctx, data, level, 8192, 4096, True, src=big.data_ptr() + 4097)[0] == want
