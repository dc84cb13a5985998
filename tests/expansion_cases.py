"""Inputs that expand: what an encoder writes when nothing compresses, at the sizes its slots and bounds are built around
(tests/test_expansion_cases_cpu.py guards the list without a GPU; tests/test_gpu_expansion.py and tests/test_gpu_dest_edges.py
hold the device to it). Deterministic, nothing read from disk, no torch.

`high(n)`     bytes in 144..255 with no trigram twice: level 1 finds no match and codes every byte in nine bits, so a packet of L
              such bytes has a size in closed form (level1_packet_bytes) within 1..2 bytes of the per-packet term of zz_bound
              (per_packet); with 112 values it still compresses at levels 2 and above.
`uniform(n)`  plain random bytes: the stored fallback at levels 2..6 (a non-final packet is L + 10 bytes against the term's L + 11),
              5.5 % growth at level 1.
`tipping`     one packet, bytes(k) + r[k:] for a fixed random r, for the five k around the one at which the oracle's block goes
              from stored to dynamic: `required >= n` of the level-2 kernel within a few bytes of its threshold.

A case of the first two families is (family, n, P): n bytes in packets of P. The lengths L are those at which 9 L + 10 bits take
every residue mod 8 (1..17), the 64-lane and 258-byte edges, and the sizes around a batch (16,384) and a full packet (32,768);
the geometries are one packet, two, three and a byte, and two with the last one a byte short -- and four packets and a byte for
tiny P, where level 0's rule for a one-byte packet (6 bytes, not len + 10) is."""
import functools
import random

import zzflate_amd as zz

LENGTHS = list(range(1, 18)) + [63, 64, 65, 255, 256, 257, 258, 259, 1000, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768]
SMALL_P = [1, 2, 3, 5, 8, 9]
FAMILIES = ["high", "uniform"]
MAX_N = 3 * 32768 + 1
DEFLATE = 2
HEADER = {0: 2, 1: 10, 2: 0}
TRAILER = {0: 4, 1: 8, 2: 0}
WBITS = {0: 15, 1: 31, 2: -15}
# (level, warm window); levels 4..6 bring their own window
COLD = [(0, 0), (1, 0), (2, 0), (3, 0)]
WARM = [(1, 258), (1, 32768), (2, 4096), (3, 32768)]
EXTENDED = [(4, 0), (5, 0), (6, 0)]
GUARD_MODES = COLD + EXTENDED + [(lvl, w) for lvl in (1, 2, 3) for w in (258, 32768)]

TIP_LENGTHS = [64, 300, 1000, 4096, 32768]
TIP_LEVELS = [2, 3, 4, 5, 6]
TIP_SEED = 7
TIP_SEARCH = 400


def _lcg(x):
    return (x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)


@functools.lru_cache(maxsize=None)
def _high(seed):
    """MAX_N bytes in 144..255, greedy: a byte whose trigram has been seen is drawn again (a 64-bit linear congruential generator,
    the same on every Python). A prefix of it is the sequence for a shorter n."""
    out, seen, x = bytearray(), set(), seed * 2 + 1
    while len(out) < MAX_N:
        x = _lcg(x)
        b = 144 + (x >> 33) % 112
        if len(out) >= 2:
            t = (out[-2] << 16) | (out[-1] << 8) | b
            if t in seen:
                continue
            seen.add(t)
        out.append(b)
    return bytes(out)


def high(n, seed=1):
    assert n <= MAX_N
    return _high(seed)[:n]


@functools.lru_cache(maxsize=None)
def _uniform(seed):
    out, x = bytearray(), seed * 2 + 1
    for _ in range(MAX_N):
        x = _lcg(x)
        out.append((x >> 33) & 255)
    return bytes(out)


def uniform(n, seed=1):
    assert n <= MAX_N
    return _uniform(seed)[:n]


def geometries():
    """(n, P), in first-seen order"""
    out = []
    for L in LENGTHS:
        for n in (L, 2 * L, 3 * L + 1, 2 * L - 1):
            if (n, L) not in out:
                out.append((n, L))
    for P in SMALL_P:
        if (4 * P + 1, P) not in out:
            out.append((4 * P + 1, P))
    return out


def cases(family=None):
    return [(f, n, P) for f in FAMILIES if family in (None, f) for n, P in geometries()]


def data(case):
    f, n, _ = case
    return high(n) if f == "high" else uniform(n)


def fmt_of(index):
    """the container format cycles with the case's index in its list"""
    return index % 3


def packets(n, P):
    """(offset, length, final) of every packet of n > 0 bytes"""
    return [(off, min(P, n - off), off + P >= n) for off in range(0, n, P)]


def level1_packet_bytes(L, final):
    """a level-1 packet of L bytes that all take nine bits and hold no match. Final: the block's 3 header bits, 9 L, the 7-bit end
    of block. Not final: the block holds L - 1 bytes and its end, then the 3 header bits of a stored block, padding, and that
    block's LEN, NLEN and the last byte -- which alone, L = 1, is the packet."""
    if final:
        return (10 + 9 * L + 7) // 8
    if L == 1:
        return 6
    return (3 + 9 * (L - 1) + 7 + 3 + 7) // 8 + 5


def per_packet(level, L):
    """the per-packet term of zz_bound, from the library: what zz_slot_stride rounds up from"""
    return zz.bound(L, zz.Format.Deflate, level, L) - 16


def stored_packet_bytes(L, final):
    """a packet whose one block fell back to stored (levels 2 and above, L <= 32768)"""
    return L + 5 if final else L + 10


def oracle_packet(oracle, d, level, off, ln, final, warm=0):
    cap = 2 * ln + 1024
    import ctypes
    b = ctypes.create_string_buffer(cap)
    w = oracle.L.zzo_packet_warm(level, d, off, ln, int(final), b, cap, warm)
    return b.raw[:w]


# ---- the stored-fallback decision at its threshold ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tip_random(L):
    rng = random.Random(TIP_SEED)
    return bytes(rng.getrandbits(8) for _ in range(L))


def tip_data(L, k):
    return bytes(k) + _tip_random(L)[k:]


def is_stored(stream, L, final):
    return len(stream) == stored_packet_bytes(L, final) and stream[0] in (0, 1)


_verdicts = {}


def tip_verdicts(oracle, L, level, final):
    """stored? for k = 0 .. min(L, TIP_SEARCH) - 1, by the oracle's packet"""
    key = (L, level, final)
    if key not in _verdicts:
        _verdicts[key] = [is_stored(oracle_packet(oracle, tip_data(L, k), level, 0, L, final), L, final) for k in range(min(L, TIP_SEARCH))]
    return _verdicts[key]


def tipping(oracle, L, level, final):
    """[(k, data)] for k* - 2 .. k* + 2, k* the first k whose block is dynamic; None when the search finds no such k"""
    v = tip_verdicts(oracle, L, level, final)
    flips = [k for k in range(1, len(v)) if v[k - 1] and not v[k]]
    if not flips:
        return None
    ks = flips[0]
    return [(k, tip_data(L, k)) for k in range(max(ks - 2, 0), min(ks + 3, L + 1))]


def tip_cells():
    return [(L, level, final) for L in TIP_LENGTHS for level in TIP_LEVELS for final in (True, False)]


def tip_stream(d, final):
    """(input, packet size) of a stream whose first packet is the case's: a non-final packet gets one more byte behind it"""
    return (d, len(d)) if final else (d + b"\xA7", len(d))


# ---- the sequential level-1 stream, whose block lengths follow from the room ------------------------------------------------

SEQ_SIZES = [300, 1000, 5000]
SEQ_SEED = {"high": 2, "uniform": 11}          # (of the first dozen seeds, the one whose windows flip three times at every size)


def seq_inputs():
    return [(f, n, high(n, SEQ_SEED[f]) if f == "high" else uniform(n, SEQ_SEED[f])) for f in FAMILIES for n in SEQ_SIZES]


def one_block_cap(n):
    """the smallest room behind the container header at which level 1 writes one block: (room - 1) * 8 / 9 - 8 >= n"""
    room = 1
    while (room - 1) * 8 // 9 - 8 < n:
        room += 1
    return room


def seq_window(oracle, d, fmt):
    """the capacities of the sweep: 40 bytes to either side of the roomy stream's length behind the header, widened upward to
    take in the one-block threshold where that lies further out (inputs that nine bits per byte overstate)"""
    roomy = len(oracle.encode(d, DEFLATE, 1))
    hi = max(roomy + 40, one_block_cap(len(d)) + 4)
    return range(roomy - 40 + HEADER[fmt], hi + HEADER[fmt])


def inflates(stream, d, fmt):
    import zlib
    try:
        o = zlib.decompressobj(WBITS[fmt])
        return stream is not None and o.decompress(stream) == d and o.eof and not o.unused_data
    except zlib.error:
        return False


def seq_expected(oracle, d, fmt, cap):
    """the oracle's level-1 stream for a destination of `cap` bytes, or None where it is no stream of d (the reference stops
    early, D9) or ends behind `cap` (the reference appends the trailer unchecked): the device then answers E_NOSPACE"""
    want = oracle.encode(d, fmt, 1, cap=cap)
    return want if want is not None and len(want) <= cap and inflates(want, d, fmt) else None
