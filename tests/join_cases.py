"""Inputs for the checksum partials, their folds and the packet join at their round edges (tests/test_join_cases_cpu.py guards
the list without a GPU, tests/test_gpu_join.py holds the device to it). Deterministic, nothing read from disk, no torch.

Every expectation is exact and has two independent sources: oracle.encode_packets gives the stream's bytes, and Python's
zlib.adler32 / zlib.crc32 of the input give the trailer and every shard partial -- a mistake the oracle shared with the kernels
could not hide behind byte equality.

Byte families (data()): `ff` is all 0xFF -- the input on which a 32-bit accumulator, a missing reduction or a product that leaves
64 bits shows; `ffnoise` is 0xFF or 0xFE per byte, so that the match finders and the fixed code give packets of varying size
while every byte still weighs 254 or more; `impulse` is zeros with one 0xFF, which pins the weight of that one position (a
packet's b is then 255 * (bytes from the impulse to the packet's end)); `random` and `zeros`.

A case is Case(group, family, n, P, arg, levels): `arg` is the seed, or the impulse's position; `levels` are the levels the
GPU tests run it at. The groups and the boundary each packet size and length family is for:

  len    P = 4096. n = 1..17 (the tail loop of wave_adler, the head and tail of coop_copy_adler), 1023 / 1024 / 1025 (one row of 64
         16-byte chunks), P - 1, P, P + 1 (the second trip of wave_adler's loop: 64 lanes * ZZ_ADLER_INFLIGHT = 4 loads * 16 bytes is
         4096), and a last packet of 1 and of P - 1 bytes.
  mod    P = 32768. n mod 65521 in {0, 1, 65520}: n = 65520, 65521, 65522, 2 * 65521 - 1, 2 * 65521, 2 * 65521 + 1 (the "bytes
         behind" remainder of the folds, adler_combine's len2 % 65521).
  part   P = 32768, one packet: wave_adler_part, three wavefronts splitting a packet by 1 KiB rows (k_encode_l1p). A wavefront's
         rows come in trips of ZZ_L1P_ADLER_U (read from zz_level1p.h: 6). One, two and three rows per wavefront are 3072, 6144 and
         9216 bytes; 3 * 64 * ZZ_L1P_ADLER_U chunks = 18,432 bytes is the last length with one trip per wavefront. Each with
         -17, -16, -1, 0, +1, +15, +16, +17 bytes (PART_LENGTHS follows from ZZ_L1P_ADLER_U; so do the impulses at 18,432 -+ 1);
         and 1024 and 2048 bytes -1, 0, +1, +16: a packet with no row for two of the wavefronts, and for one.
  crc    gzip, n = 2 P + 777 (a short last packet on the slicing path). P = 1000 and 32767 take the slicing path throughout;
         1024, 2048, 3072, 5120, 9216 and 32768 give 1, 2, 3, 5, 9 and 32 rows of 256 bytes per quarter: the single row, the plain
         loop, the unrolled-by-8 loop with a remainder (9) and without (32: three unrolled trips, seven plain rows, the last row).
         Impulses at the word, row, eight-row and quarter edges of P = 32768.
  round  the join's rounds, with tiny packets: npk = 1023, 1024, 1025, 2049 (k_cks_reduce's run of 1, 2 and 3 packets per thread;
         the CRC grid of 2048) at P = 64, 33, 16, 24; npk = 4095, 4096, 4097, 8193 (k_scan_sizes' rounds of 4096 packets and its
         carry) at P = 17, 16, 48, 31; npk = 16,385 at P = 8 (k_encode_l0's grid of 16,384); npk = 65,537 and 65,538 at P = 3
         (k_compact's grid of 65,536; levels 0 and 1) and 65,537 at P = 7, the smallest packet whose level-1 streams take three
         sizes on `ffnoise` (at P = 3 every packet takes 9 bytes); and `ff` at P = 256 with 65,800 packets at level 0: every
         packet's a is 65,280, so their sum passes 2^32 -- the only place a fold of k_cks_reduce that forgot to reduce a would
         show in 32 bits.
"""
import collections
import os
import random
import re
import struct
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zzflate_amd", "csrc")
ADLER_MOD = 65521
WBITS = {0: 15, 1: 31, 2: -15}
HEADER = {0: b"\x78\x01", 1: b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff", 2: b""}

Case = collections.namedtuple("Case", "group family n P arg levels")


def header_define(header, name):
    """the default of a tuning knob, as its header spells it"""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"^#define\s+%s\s+(\d+)" % re.escape(name), text, re.M)
    assert m, (header, name)
    return int(m.group(1))


L1P_ADLER_U = header_define("zz_level1p.h", "ZZ_L1P_ADLER_U")
ADLER_INFLIGHT = header_define("zz_checksum.h", "ZZ_ADLER_INFLIGHT")
WAVE = 64
PARTS = 3                                      # wavefronts that split a packet's Adler-32 sums in k_encode_l1p
ROW = WAVE * 16                                # bytes one wavefront loads at a time: 64 chunks of 16 bytes

_NOISE = bytes(0xFF if b & 1 else 0xFE for b in range(256))


def _random_bytes(n, seed):
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little") if n else b""


def data(c):
    """the case's input"""
    if c.family == "ff":
        return b"\xFF" * c.n
    if c.family == "zeros":
        return bytes(c.n)
    if c.family == "random":
        return _random_bytes(c.n, 7919 * c.arg + c.n)
    if c.family == "ffnoise":
        return _random_bytes(c.n, 104729 * c.arg + c.n).translate(_NOISE)
    if c.family == "impulse":
        b = bytearray(c.n)
        b[c.arg] = 0xFF
        return bytes(b)
    raise ValueError(c.family)


def trailer(d, fmt):
    """the container's trailer by Python's zlib alone"""
    if fmt == 0:
        return struct.pack(">I", zlib.adler32(d))
    if fmt == 1:
        return struct.pack("<II", zlib.crc32(d), len(d) & 0xFFFFFFFF)
    return b""


def partial(d, fmt):
    """what encode_shard reports for the bytes d: the Adler-32 with start value 0 as (b << 16) | a -- the value v for which
    combine(1, v, len(d)) is zlib.adler32(d) --, or the plain CRC-32"""
    if fmt == 1:
        return zlib.crc32(d)
    ad = zlib.adler32(d)                       # a = 1 + sum d, b = n + sum (n - i) d_i
    a, b = ad & 0xFFFF, ad >> 16
    return (((b - len(d)) % ADLER_MOD) << 16) | ((a - 1) % ADLER_MOD)


def inflates(s, d, fmt):
    """zlib takes the whole of s, trailer included, and gives d"""
    try:
        o = zlib.decompressobj(WBITS[fmt])
        return o.decompress(s) == d and o.eof and o.unused_data == b""
    except zlib.error:
        return False


def npk(c):
    return -(-c.n // c.P)


def last_packet(c):
    return c.n - (npk(c) - 1) * c.P


ALL = (0, 1, 2, 3)
LEN_P = 4096
LEN_LENGTHS = list(range(1, 18)) + [1023, 1024, 1025, LEN_P - 1, LEN_P, LEN_P + 1, 2 * LEN_P + 1, 3 * LEN_P - 1]
LEN_IMPULSE_N = 3 * LEN_P + 5
LEN_IMPULSES = [0, LEN_IMPULSE_N - 1, 15, 17, 1023, 1024, 1025, LEN_P - 1, LEN_P, LEN_P + 1, 2 * LEN_P - 1, 2 * LEN_P]
MOD_LENGTHS = [ADLER_MOD - 1, ADLER_MOD, ADLER_MOD + 1, 2 * ADLER_MOD - 1, 2 * ADLER_MOD, 2 * ADLER_MOD + 1]
# follows from ZZ_L1P_ADLER_U: the last entry is the most bytes the three wavefronts sum with one trip of their loops each
PART_EDGES = [PARTS * ROW, 2 * PARTS * ROW, 3 * PARTS * ROW, PARTS * ROW * L1P_ADLER_U]
PART_LENGTHS = sorted({e + k for e in PART_EDGES for k in (-17, -16, -1, 0, 1, 15, 16, 17)} |
                      {e + k for e in (ROW, 2 * ROW) for k in (-1, 0, 1, 16)})     # one and two wavefronts without a row
PART_IMPULSES = sorted({0, 32767, 15, 17} | {ROW * k + s for k in (1, 2, 3) for s in (-1, 0, 1)} |
                       {e + s for e in PART_EDGES for s in (-1, 0, 1)})
CRC_PACKETS = [1000, 1024, 2048, 3072, 5120, 9216, 32767, 32768]
CRC_IMPULSES = [0, 3, 4, 255, 256, 2047, 2048, 8192 - 257, 8192 - 256, 8191, 8192, 3 * 8192 - 1, 3 * 8192, 32767, 32768, 2 * 32768 + 776]
# (npk, P, last packet, families, levels)
ROUNDS = [
    (1023, 64, 1, ("ff", "ffnoise"), ALL), (1024, 33, 32, ("ff", "ffnoise"), (0, 1)), (1025, 16, 16, ("ff", "ffnoise", "random"), ALL),
    (2049, 24, 5, ("ff", "ffnoise"), (0, 1)),
    (4095, 17, 17, ("ffnoise",), (0, 1)), (4096, 16, 1, ("ff", "ffnoise"), (0, 1)), (4097, 48, 47, ("ff", "ffnoise", "random"), ALL),
    (8193, 31, 7, ("ff", "ffnoise"), ALL),
    (16385, 8, 3, ("ff", "ffnoise"), (0, 1)),
    (65537, 3, 3, ("ff", "ffnoise"), (0, 1)), (65538, 3, 1, ("ffnoise",), (0, 1)), (65537, 7, 2, ("ffnoise",), (1,)),
    (65800, 256, 256, ("ff",), (0,)),
]


def cases():
    out = []
    for fam in ("ff", "ffnoise", "random", "zeros"):
        out += [Case("len", fam, n, LEN_P, 1, ALL) for n in LEN_LENGTHS]
    out += [Case("len", "impulse", LEN_IMPULSE_N, LEN_P, p, ALL) for p in LEN_IMPULSES]
    for fam in ("ff", "ffnoise"):
        out += [Case("mod", fam, n, 32768, 2, ALL) for n in MOD_LENGTHS]
    for fam in ("ff", "ffnoise"):
        out += [Case("part", fam, n, 32768, 3, ALL) for n in PART_LENGTHS]
    out += [Case("part", "impulse", 32768, 32768, p, ALL) for p in PART_IMPULSES]
    for P in CRC_PACKETS:
        out += [Case("crc", fam, 2 * P + 777, P, 4, ALL) for fam in ("ff", "random")]
    out += [Case("crc", "impulse", 2 * 32768 + 777, 32768, p, ALL) for p in CRC_IMPULSES]
    for k, P, last, fams, levels in ROUNDS:
        out += [Case("round", fam, (k - 1) * P + last, P, 5, levels) for fam in fams]
    return out


CASES = cases()


def group(name, level=None):
    return [c for c in CASES if c.group == name and (level is None or level in c.levels)]


def case_id(c):
    return f"{c.group}-{c.family}-n{c.n}-P{c.P}-{c.arg}"


# ---- what the boundaries are, computed from a case (the guards of test_join_cases_cpu.py) -------------------------------

def adler_part_rows(n, part):
    """rows of 64 chunks that wavefront `part` of three sums in wave_adler_part for a packet of n bytes"""
    nchunks = n >> 4
    return sum(1 for r in range(nchunks // WAVE + 1) if (r * PARTS + part) * WAVE < nchunks)


def adler_part_trips(n, part):
    return -(-adler_part_rows(n, part) // L1P_ADLER_U)


def wave_adler_trips(n):
    return -(-(n >> 4) // (WAVE * ADLER_INFLIGHT))


def crc_rows(P):
    """rows of 256 bytes per quarter on the fast path of crc32_packets_run; None on the slicing path"""
    return P // 4 // 256 if P % 1024 == 0 and P >= 1024 else None


def crc_loops(rows):
    """(trips of the unrolled-by-8 loop, trips of the plain loop) in front of the last row"""
    r = u = p = 0
    while r + 8 < rows:
        r += 8
        u += 1
    while r + 1 < rows:
        r += 1
        p += 1
    return u, p


def reduce_run(c):
    """packets per thread of k_cks_reduce"""
    return -(-npk(c) // 1024)


def scan_rounds(c):
    return -(-npk(c) // 4096)


# ---- the batch: items of 1, 63, 64, 65 and 130 packets, families mixed -----------------------------------------------
BATCH_P = 512
BATCH_PACKETS = [1, 63, 64, 65, 130]


def batch_items():
    """16 items: the five packet counts over `ff`, `impulse` and `random`, the last packet short in every second one"""
    out = []
    for i in range(16):
        k = BATCH_PACKETS[i % 5]
        n = k * BATCH_P - (0 if i % 2 else 37 % (BATCH_P - 1))
        fam = ("ff", "impulse", "random")[i % 3]
        out.append(Case("batch", fam, n, BATCH_P, (n - 1 - i) if fam == "impulse" else i, ALL))
    return out


# ---- the batch decoder's item routine: zi_adler_lanes' outer loop takes a second trip above 65,536 bytes a lane -----------
ITEM_LENGTHS_ONE_LANE = [65535, 65536, 65537, 200000]
ITEM_LENGTH_64_LANES = 64 * 65536 + ADLER_MOD + 3


def item_stream(family, n, fmt):
    """(input, zlib's own level-9 stream of it: a few KB)"""
    d = data(Case("item", family, n, 32768, 9, ()))
    co = zlib.compressobj(9, zlib.DEFLATED, WBITS[fmt])
    return d, co.compress(d) + co.flush()


def bad_trailers(s, fmt):
    """the stream with its trailer off by one: (what, stream) for the Adler-32's low and high half, or the CRC-32 and ISIZE"""
    def bump(at, width, big):
        b = bytearray(s)
        v = int.from_bytes(b[at:at + width], "big" if big else "little")
        b[at:at + width] = ((v + 1) % (1 << (8 * width))).to_bytes(width, "big" if big else "little")
        return bytes(b)
    if fmt == 0:
        return [("adler low half", bump(len(s) - 2, 2, True)), ("adler high half", bump(len(s) - 4, 2, True))]
    if fmt == 1:
        return [("crc", bump(len(s) - 8, 4, False)), ("isize", bump(len(s) - 4, 4, False))]
    return []
