"""Inputs and expectations for the tests of zz_encode_members_device (tests/test_members_write_cpu.py guards the list without
a GPU, tests/test_gpu_encode_members.py holds the device to it). The yardstick is the format rule restated in Python from
the oracle: a member is an 18-byte header announcing its own length, the raw-deflate stream the oracle writes for its block
alone -- or the block's level-0 stream where that is shorter -- and CRC-32 and ISIZE."""
import functools
import struct
import zlib

import members_cases as mc
from conftest import synth

BLOCK = 65280                        # zz.MEMBERS_BLOCK, restated
PACKET = 32768
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")         # then BSIZE = the member's bytes - 1, little-endian
LEVELS = [0, 1, 2, 3]
DEFLATE = 2                          # the oracle's raw format


def expected(oracle, data, level, B, P, eof):
    """(file, member offsets (members + 1 of them), stored flags) by the rule"""
    out, offsets, stored = bytearray(), [], []
    for at in range(0, len(data), B):
        block = data[at:at + B]
        body = oracle.encode_packets(block, DEFLATE, level, P)
        fallback = body if level == 0 else oracle.encode_packets(block, DEFLATE, 0, P)
        took = len(body) > len(fallback)
        if took:
            body = fallback
        total = len(HEADER) + 2 + len(body) + 8
        assert total <= 65536, "the rule keeps every member inside BSIZE"
        offsets.append(len(out))
        stored.append(took)
        out += HEADER + struct.pack("<H", total - 1) + body + struct.pack("<II", zlib.crc32(block), len(block))
    offsets.append(len(out))
    if eof:
        out += mc.EOF_BLOCK
    return bytes(out), offsets, stored


def stored_stream_bytes(n, P):
    """S: bytes of the level-0 stream of n > 0 input bytes in packets of P (a packet that is not the last ends with a stored
    block of its last byte, so that it ends on a byte boundary with no final bit: n + 10, or 6 for a one-byte packet)"""
    npk = -(-n // P)
    return (npk - 1) * (P + 10 if P > 1 else 6) + (n - (npk - 1) * P) + 5


def bound(n, B=BLOCK, P=PACKET, eof=True):
    """zz_encode_members_bound restated: every member stored; None for sizes the call refuses"""
    B, P = B or BLOCK, P or PACKET
    if B > 65536 or P > 32768 or 26 + stored_stream_bytes(B, P) > 65536:
        return None
    m = -(-n // B)
    total = 0 if m == 0 else (m - 1) * (26 + stored_stream_bytes(B, P)) + 26 + stored_stream_bytes(n - (m - 1) * B, P)
    return total + (28 if eof else 0)


def members_of(file):
    """(offset, bytes) of every member, by the BSIZE chain"""
    out, at = [], 0
    while at < len(file):
        assert file[at:at + 16] == HEADER, at
        size = struct.unpack_from("<H", file, at + 16)[0] + 1
        out.append((at, size))
        at += size
    assert at == len(file)
    return out


def text(n, seed=0):
    return mc.text(n, seed)


def mixed(n_text, n_random, n_tail, seed):
    return text(n_text, seed) + synth("random", n_random, seed) + text(n_tail, seed + 1)


def threshold_data(r):
    """one block of (8192, 4096): r random bytes, then text; a short text block behind it"""
    return synth("random", 8192, 77)[:r] + text(8192, 5)[r:] + text(1000, 6)


@functools.lru_cache(maxsize=None)
def _threshold(oracle):
    """r with D <= S at r and D > S at r + 1, level 1 at (8192, 4096): bisection between all text (compressed) and all random
    (stored) ends on such a neighbouring pair whether or not D is monotone in r"""
    def took(r):
        return expected(oracle, threshold_data(r), 1, 8192, 4096, False)[2][0]
    lo, hi = 0, 8192
    assert not took(lo) and took(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if took(mid):
            hi = mid
        else:
            lo = mid
    return lo


def threshold_pair(oracle):
    r = _threshold(oracle)
    return threshold_data(r), threshold_data(r + 1)


@functools.lru_cache(maxsize=None)
def cases(oracle):
    """(name, data, B, P, eof)"""
    B = BLOCK
    out = []
    long_text = text(3 * B + 777, 1)
    for k, n in enumerate((0, 1, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 777)):
        out.append((f"text, n = {n}", long_text[:n], B, PACKET, k % 3 != 2))
    for kind in ("random", "zeros", "runs"):
        out.append((f"{kind}, n = 2B + 1", synth(kind, 2 * B + 1, 3), B, PACKET, kind != "zeros"))
    out.append(("text, 100000 random bytes, text", mixed(40000, 100000, 60000, 2), B, PACKET, True))
    out.append(("text, 100000 random bytes, text; packets of 4096", mixed(40000, 100000, 60000, 4), B, 4096, False))
    out.append(("(4096, 4096) over 300000 bytes", mixed(100000, 100000, 100000, 6), 4096, 4096, True))
    out.append(("(777, 300) over 50000 bytes", text(20000, 8) + synth("random", 10000, 8) + synth("runs", 20000, 8), 777, 300, True))
    out.append(("(8192, 4096)", text(30000, 9) + synth("random", 30000, 9) + bytes(10000) + text(30001, 10), 8192, 4096, False))
    lo, hi = threshold_pair(oracle)
    out.append(("(8192, 4096), the last r that compresses", lo, 8192, 4096, True))
    out.append(("(8192, 4096), the first r that is stored", hi, 8192, 4096, True))
    return out


@functools.lru_cache(maxsize=None)
def expected_case(oracle, index, level):
    """expected(...) of cases(oracle)[index], computed once and shared"""
    _, data, B, P, eof = cases(oracle)[index]
    return expected(oracle, data, level, B, P, eof)
