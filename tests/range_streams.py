"""What the range-decode tests share (test_inflate_range_cpu.py on the host, test_gpu_decode_range.py on the device): the list
of ranges to read from a stream, and hand-made packet-mode streams whose pointer chains are known by construction -- fixed-Huffman
blocks from a small bit writer, every packet closed by the one-byte stored block, P = 1000."""
import random
import zlib

HAND_P = 1000
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def ranges_for(L, P, seed):
    """(first, nbytes) pairs for a stream of L > 0 decoded bytes in packets of P: the edges, whole packets, 50 seeded random
    ranges, ranges clipped at the end, and starts behind the end but inside the last packet's span (0 bytes)."""
    npk = max(1, (L + P - 1) // P)
    out = [(0, 1), (0, L), (L - 1, 1)]
    if L > P:
        out.append((P - 1, 2))
    out += [(k * P, P) for k in sorted({1 % npk, npk // 2, npk - 1})]
    rng = random.Random(seed)
    for _ in range(50):
        first = rng.randrange(L)
        n = rng.choice((1, rng.randrange(1, 300), rng.randrange(1, 3 * P), rng.randrange(1, L + 1)))
        out.append((first, min(n, L - first)))
    out += [(L - min(L, 10), 100), (rng.randrange(L), 2 * L), (0, (1 << 64) - 1)]       # clipped
    if L < npk * P:
        out += [(L, 5), (npk * P - 1, 1)]                                              # behind the end: nothing
    return out


def want(data, first, nbytes):
    return data[first: first + nbytes]


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):
        self.v |= v << self.n
        self.n += n

    def huff(self, code, n):          # Huffman codes go most significant bit first
        self.put(int(format(code, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        self.n = (self.n + 7) & ~7

    def nbytes(self):
        assert self.n % 8 == 0
        return self.n // 8

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed_sym(b, sym):
    if sym < 144:
        b.huff(0x30 + sym, 8)
    elif sym < 256:
        b.huff(0x190 + sym - 144, 9)
    elif sym < 280:
        b.huff(sym - 256, 7)
    else:
        b.huff(0xC0 + sym - 280, 8)


def fixed_match(b, length, dist):
    li = max(i for i, v in enumerate(LEN_BASE) if v <= length)
    if length == 258:
        li = 28
    fixed_sym(b, 257 + li)
    b.put(length - LEN_BASE[li], LEN_EXTRA[li])
    di = max(i for i, v in enumerate(DIST_BASE) if v <= dist)
    b.huff(di, 5)
    b.put(dist - DIST_BASE[di], DIST_EXTRA[di])


def packet(b, body, closing, final):
    """one packet: a fixed-Huffman block of literals (ints) and (length, distance) matches, then the stored block of one byte"""
    b.put(0, 1); b.put(1, 2)
    for t in body:
        if isinstance(t, tuple):
            fixed_match(b, *t)
        else:
            fixed_sym(b, t)
    fixed_sym(b, 256)
    b.put(1 if final else 0, 1); b.put(0, 2); b.align()
    b.put(1, 16); b.put(0xFFFE, 16); b.put(closing, 8)


def hand_stream(kind, packets=44):
    """(zlib stream, index, decoded bytes or None) of the hand-made stream `kind`:
    a: packet 0 is literals; every later packet is matches at distance P, so every byte's chain runs to packet 0
    b: the same, but packet 37 is literals again: chains from behind it end there
    c: a: with a match in packet 0 whose source lies in front of the stream (not a valid stream)"""
    P = HAND_P
    rng = random.Random(ord(kind))
    b = Bits()
    index, data = [0], bytearray()
    copies = [(258, P), (258, P), (258, P), (P - 1 - 3 * 258, P)]
    for k in range(packets):
        closing = rng.getrandbits(8)
        if k == 0 or (kind == "b" and k == 37):
            lits = bytes(rng.getrandbits(8) for _ in range(P - 1))
            body = list(lits)
            if kind == "c":
                body[10:268] = [(258, 11)]                     # at position 10 a match from one byte in front of the stream
        else:
            lits, body = bytes(data[-P: -1]), copies
        packet(b, body, closing, k == packets - 1)
        index.append(b.nbytes())
        data += lits + bytes([closing])
    data = None if kind == "c" else bytes(data)
    return b"\x78\x01" + b.bytes() + zlib.adler32(data or b"").to_bytes(4, "big"), index, data
