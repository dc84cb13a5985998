"""What the decode conformance tests share (test_inflate_conformance_cpu.py on the host, test_gpu_decode_conformance.py on the
device): raw DEFLATE streams whose verdict -- these bytes, or not a stream -- comes from Python's zlib when the case is built,
never from the code under test.

  boundary_cases()   hand-made streams at the edges of RFC 1951: every length and distance code at both ends of its extra bits,
                     overlapping copies around the 64-lane stride, distance limits, and every rule of the fixed, dynamic and
                     stored block headers, each with the verdict it is meant to have (zlib must agree when it is built)
  mutations(n, seed) zlib's own streams with a flipped bit, replaced bytes or a cut
  foreign_packets()  packet-mode streams written by zlib: dynamic codes, distances up to 32 KiB, chains through every packet
"""
import functools
import os
import random
import zlib

from range_streams import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, Bits, fixed_match, fixed_sym

CORPUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpus")
CAP = 65536                   # the destination of a stream that is not expected to decode
ROOMY = 1 << 18               # the cap under which a hand-made stream gets its verdict (none decodes to more)
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
NOT_MEANT = "the hand-made stream is not what it means to be"


def verdict(raw, cap):
    """zlib's word on the raw stream `raw` decoded into `cap` bytes: ("ok", bytes), ("big", None) or ("bad", None)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw, cap + 1)
    except zlib.error:
        return "bad", None
    if len(out) > cap:
        return "big", None
    if d.eof and not d.unused_data:
        return "ok", out
    return "bad", None                                   # truncated, or bytes behind the final block


def corpus(name):
    with open(os.path.join(CORPUS, name), "rb") as f:
        return f.read()


# ---- the bit writer's vocabulary -------------------------------------------------------------------------------------------
def canonical(lens):
    codes, code = [0] * len(lens), 0
    for L in range(1, 16):
        for s, l in enumerate(lens):
            if l == L:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def kraft(lens):
    """the code space the lengths take, in units of 2^-15 (a complete code: 32768)"""
    return sum(1 << (15 - l) for l in lens if l)


def balanced(symbols):
    """a complete code over `symbols` (two or more): lengths k - 1 and k"""
    n = len(symbols)
    k = max(1, (n - 1).bit_length())
    a = (1 << k) - n
    return {s: (k - 1 if i < a else k) for i, s in enumerate(symbols)}


def length_symbol(length, top=False):
    """(symbol index 0..28, extra value) of a match length; `top`: 258 as symbol 284 with all extra bits set"""
    if length == 258 and not top:
        return 28, 0
    li = max(i for i, v in enumerate(LEN_BASE[:28]) if v <= length)
    return li, length - LEN_BASE[li]


def dist_symbol(dist):
    di = max(i for i, v in enumerate(DIST_BASE) if v <= dist)
    return di, dist - DIST_BASE[di]


class Dynamic:
    """a dynamic block's header written into `b`, and the writers of its symbols. `cl_syms`: the code-length symbols to send
    ((symbol, extra value) pairs; default: every length as itself, no repeats); `hlit` / `hdist`: the counts the header claims."""

    def __init__(self, b, final, lit, dist, cl_lens=None, hclen=19, cl_syms=None, hlit=None, hdist=None):
        self.b = b
        lit, dist = list(lit), list(dist)
        if cl_syms is None:
            cl_syms = [(l, 0) for l in lit + dist]
        if cl_lens is None:
            used = sorted({s for s, _ in cl_syms} | {0})
            cl_lens = balanced(used if len(used) > 1 else [0, 18])
        assert set(cl_lens) <= set(ORDER[:hclen])
        b.put(1 if final else 0, 1); b.put(2, 2)
        b.put((len(lit) if hlit is None else hlit) - 257, 5)
        b.put((len(dist) if hdist is None else hdist) - 1, 5)
        b.put(hclen - 4, 4)
        for i in range(hclen):
            b.put(cl_lens.get(ORDER[i], 0), 3)
        clc = canonical([cl_lens.get(s, 0) for s in range(19)])
        for s, extra in cl_syms:
            b.huff(clc[s], cl_lens[s])
            if s >= 16:
                b.put(extra, (2, 3, 7)[s - 16])
        self.lit, self.dist = lit, dist
        self.lc, self.dc = canonical(lit), canonical(dist)

    def sym(self, s):
        assert self.lit[s], s
        self.b.huff(self.lc[s], self.lit[s])

    def match(self, length, dist, top=False):
        li, le = length_symbol(length, top)
        self.sym(257 + li)
        self.b.put(le, LEN_EXTRA[li])
        di, de = dist_symbol(dist)
        assert self.dist[di], di
        self.b.huff(self.dc[di], self.dist[di])
        self.b.put(de, DIST_EXTRA[di])


class Fixed:
    """the same face over a fixed block"""

    def __init__(self, b, final):
        self.b = b
        b.put(1 if final else 0, 1); b.put(1, 2)

    def sym(self, s):
        fixed_sym(self.b, s)

    def match(self, length, dist, top=False):
        if top:
            li, le = length_symbol(length, True)
            fixed_sym(self.b, 257 + li)
            self.b.put(le, LEN_EXTRA[li])
            di, de = dist_symbol(dist)
            self.b.huff(di, 5)
            self.b.put(de, DIST_EXTRA[di])
        else:
            fixed_match(self.b, length, dist)


def stored(b, final, payload, nlen=None):
    b.put(1 if final else 0, 1); b.put(0, 2); b.align()
    b.put(len(payload), 16); b.put((len(payload) ^ 0xFFFF) if nlen is None else nlen, 16)
    for c in payload:
        b.put(c, 8)


def complete(lens, free):
    """fills the symbols `free` of `lens` (now 0) with lengths that make the code complete: the space the others leave, as that
    many powers of two (its binary digits, the largest split in two until there are enough)"""
    lens = list(lens)
    room = 32768 - kraft(lens)
    terms = sorted(1 << i for i in range(16) if room >> i & 1)
    assert 0 < len(terms) <= len(free) <= room
    while len(terms) < len(free):
        big = terms.pop()
        terms += [big // 2, big // 2]
        terms.sort()
    for s, t in zip(free, reversed(terms)):
        lens[s] = 16 - t.bit_length()
    assert kraft(lens) == 32768 and all(1 <= lens[s] <= 15 for s in free)
    return lens


# ---- boundary cases -------------------------------------------------------------------------------------------------------
def _length_distance_walk(rng):
    """every length symbol at its smallest and largest extra bits against every distance code at its smallest and largest extra
    bits, behind 32 KiB of literals: four streams of fixed blocks, four of dynamic blocks whose match symbols have 9..15 bits"""
    pairs = []
    for li in range(29):
        for le in sorted({0, (1 << LEN_EXTRA[li]) - 1}):
            for di in range(30):
                for de in sorted({0, (1 << DIST_EXTRA[di]) - 1}):
                    pairs.append((LEN_BASE[li] + le, li == 27 and le == 31, DIST_BASE[di] + de))
    assert len(pairs) == (29 * 2 - 9) * (30 * 2 - 4)         # (symbols without extra bits have one end)
    # the dynamic code: length symbols 257..285 take 9..15 bits, the distance codes 5..15; literals and the end of block fill up
    lit = [0] * 286
    for i in range(29):
        lit[257 + i] = 9 + i % 7
    lit = complete(lit, list(range(257)))
    dist = [0] * 30
    for i in range(30):
        dist[i] = (15, 14, 13, 12, 11)[i % 5] if i >= 10 else 0
    dist = complete(dist, list(range(10)))
    assert max(lit[257:]) == 15 and min(lit[257:]) == 9 and max(dist) == 15
    out = []
    parts = 4
    for kind in ("fixed", "dynamic"):
        for p in range(parts):
            prefix = bytes(rng.getrandbits(8) for _ in range(32768))
            b = Bits()
            blk = Fixed(b, True) if kind == "fixed" else Dynamic(b, True, lit, dist)
            for c in prefix:
                blk.sym(c)
            for j, (length, top, d) in enumerate(pairs[p::parts]):
                blk.match(length, d, top)
                if j % 16 == 0:
                    blk.sym(rng.getrandbits(8))
            blk.sym(256)
            out.append((f"walk_{kind}_{p}", b.bytes(), "ok"))
    return out


OVERLAP_DISTS = list(range(1, 71)) + [127, 128, 129, 257, 258, 259]
OVERLAP_LENS = [3, 4, 63, 64, 65, 127, 128, 129, 257, 258]


def _overlapping_copies(rng):
    out = []
    for d in OVERLAP_DISTS:
        b = Bits()
        blk = Fixed(b, True)
        for _ in range(d):                                   # the seed of the first copy: as long as the distance
            blk.sym(rng.getrandbits(8))
        for n in OVERLAP_LENS:
            blk.match(n, d)
            for _ in range(5):                               # a short literal seed in front of the next one
                blk.sym(rng.getrandbits(8))
        blk.sym(256)
        out.append((f"overlap_dist{d}", b.bytes(), "ok"))
    return out


def _distance_limits(rng):
    out = []
    # 32769 is not a distance DEFLATE can write: at the far end the pair is distance 32768 behind 32768 and behind 32767 literals
    for produced, dist, meant in ((5, 5, "ok"), (5, 6, "bad"), (32768, 32768, "ok"), (32767, 32768, "bad"), (32769, 32768, "ok")):
        b = Bits()
        blk = Fixed(b, True)
        for _ in range(produced):
            blk.sym(rng.getrandbits(8))
        blk.match(258, dist)
        blk.sym(256)
        out.append((f"distance_{dist}_behind_{produced}", b.bytes(), meant))
    return out


def _fixed_block(rng):
    out = []
    for s in (286, 287):
        b = Bits()
        blk = Fixed(b, True)
        # (what follows reads as six extra bits and distance 1, should a decoder take the symbol for a length)
        blk.sym(97); blk.sym(s); b.put(0, 6); b.huff(0, 5); blk.sym(256)
        out.append((f"fixed_symbol_{s}", b.bytes(), "bad"))
    for dc in (30, 31):
        b = Bits()
        blk = Fixed(b, True)
        for _ in range(4):
            blk.sym(97)
        blk.sym(257); b.huff(dc, 5); blk.sym(256)
        out.append((f"fixed_distance_code_{dc}", b.bytes(), "bad"))
        # .. and behind enough bytes for the distance the code would stand for (32769, 49153) with its fourteen extra bits
        b = Bits()
        blk = Fixed(b, True)
        for _ in range(50000):
            blk.sym(rng.getrandbits(8))
        blk.sym(257); b.huff(dc, 5); b.put(0, 14); blk.sym(256)
        out.append((f"fixed_distance_code_{dc}_behind_50000", b.bytes(), "bad"))
    b = Bits()
    Fixed(b, True).sym(256)
    out.append(("fixed_empty", b.bytes(), "ok"))
    # the bytes end inside a match's extra bits: of the length (symbol 284, five bits), of the distance (code 10, four bits)
    for which in ("length", "distance"):
        for lead in range(48, 80):
            b = Bits()
            blk = Fixed(b, True)
            for i in range(lead):
                blk.sym(200 if i % 3 == 0 else 97)               # nine- and eight-bit literals: every bit offset comes by
            fixed_sym(b, 284)
            lo = b.n; b.put(17, 5); hi = b.n
            b.huff(10, 5)
            if which == "distance":
                lo = b.n; b.put(9, 4); hi = b.n
            else:
                b.put(9, 4)
            blk.sym(256)
            whole = b.bytes()
            cut = (lo + 7) // 8 if lo % 8 else lo // 8 + 1
            if lo < cut * 8 < hi:
                assert verdict(whole, ROOMY)[0] == "ok", NOT_MEANT
                out.append((f"fixed_ends_inside_{which}_extra_bits", whole[:cut], "bad"))
                break
        else:
            raise AssertionError("no byte boundary inside the extra bits")
    return out


def _dynamic_header(rng):
    out = []
    base_lit = [0] * 257
    base_lit[97], base_lit[256] = 1, 1                       # 'a' and the end of block, one bit each

    def simple(name, meant, tail=True, **kw):
        b = Bits()
        blk = Dynamic(b, True, kw.pop("lit", base_lit), kw.pop("dist", [0]), **kw)
        if tail:
            for _ in range(6):
                blk.sym(97)
            blk.sym(256)
        else:
            b.put(0, 64)
        out.append((name, b.bytes(), meant))

    # HLIT and HDIST above what RFC 1951 allows: the lengths that follow fill the claimed counts, and the block is whole
    for hlit in (287, 288):
        simple(f"hlit_{hlit}", "bad", lit=base_lit + [0] * (hlit - 257), hlit=hlit)
    for hdist in (31, 32):
        simple(f"hdist_{hdist}", "bad", dist=[1] + [0] * (hdist - 1), hdist=hdist)
    # HCLEN 4: only 16, 17, 18 and 0 can have a code, so every length is 0 and there is no end of block
    simple("hclen_4", "bad", tail=False, cl_lens={0: 1, 18: 1}, hclen=4, cl_syms=[(18, 127), (18, 109)])
    # HCLEN 5..19: the code-length symbol the count just lets in is used (8, 7, 9, 6, 10, .. as ORDER has them), by a complete
    # literal code of the lengths the header can say: 256 codes of eight bits with some of them traded for the new length
    for hclen in range(5, 20):
        v = ORDER[hclen - 1]
        if v == 8:
            ls = [8] * 256
        elif v < 8:
            ls = [v] + [8] * (256 - (1 << (8 - v)))
        else:
            ls = list(range(9, v + 1)) + [v] + [8] * 255
        assert kraft(ls) == 32768 and set(ls) <= set(ORDER[3:hclen])
        lit = [0] * max(257, len(ls) + 1)
        lit[256] = ls[0]
        free = [s for s in range(len(lit)) if s != 256]
        for s, l in zip(free, ls[1:]):
            lit[s] = l
        while len(lit) > 257 and lit[-1] == 0:
            lit.pop()
        b = Bits()
        blk = Dynamic(b, True, lit, [0], hclen=hclen)
        text = [s for s in range(256) if lit[s]]
        for s in text[:40] + text[-40:]:
            blk.sym(s)
        blk.sym(256)
        out.append((f"hclen_{hclen}", b.bytes(), "ok"))
    # repeats
    simple("repeat_16_first", "bad", tail=False, cl_lens={16: 1, 1: 1}, cl_syms=[(16, 0)] + [(1, 0)] * 8)
    # 97 zeros, 'a', 158 zeros, the end of block, then a repeat of three zeros where one length is left: a whole block but for that
    simple("repeat_overruns_the_counts", "bad", cl_syms=[(18, 86), (1, 0), (18, 127)] + [(0, 0)] * 20 + [(1, 0), (17, 0)])
    lit = [0] * 258
    lit[97], lit[256], lit[257] = 1, 2, 2
    cl_syms = [(18, 86), (1, 0), (18, 127), (0, 0)] + [(0, 0)] * 19 + [(2, 0), (16, 2)]      # 256 is sent, then 2 x 5: 257 and four distances
    b = Bits()
    blk = Dynamic(b, True, lit, [2, 2, 2, 2], cl_lens={0: 2, 1: 3, 2: 3, 16: 2, 18: 2}, cl_syms=cl_syms)
    for _ in range(5):
        blk.sym(97)
    blk.match(3, 2); blk.match(3, 4)
    blk.sym(256)
    out.append(("repeat_spans_literals_and_distances", b.bytes(), "ok"))
    # over-subscribed codes
    simple("oversubscribed_code_length_code", "bad", tail=False, cl_lens={0: 1, 1: 1, 18: 1}, cl_syms=[(0, 0)] * 258)
    three = list(base_lit); three[98] = 1
    simple("oversubscribed_literal_code", "bad", tail=False, lit=three)
    simple("oversubscribed_distance_code", "bad", tail=False, dist=[1, 1, 1])
    # incomplete codes: refused unless they are the single one-bit code (the blocks are whole, and use only codes that exist)
    two = [0] * 257; two[97], two[256] = 2, 2
    simple("incomplete_literal_code", "bad", lit=two)
    simple("incomplete_distance_code", "bad", dist=[2, 2])
    simple("incomplete_distance_code_one_long", "bad", dist=[2])
    only_end = [0] * 257; only_end[256] = 1
    b = Bits()
    Dynamic(b, False, only_end, [0]).sym(256)
    blk = Fixed(b, True)
    for c in b"ok":
        blk.sym(c)
    blk.sym(256)
    out.append(("one_bit_literal_code", b.bytes(), "ok"))
    lit3 = [0] * 258; lit3[97], lit3[256], lit3[257] = 1, 2, 2
    for which in (0, 1):                                     # the one distance code as symbol 0 and as symbol 1
        b = Bits()
        blk = Dynamic(b, True, lit3, [1] if which == 0 else [0, 1])
        for _ in range(5):
            blk.sym(97)
        blk.sym(257); b.huff(0, 1)
        blk.sym(256)
        out.append((f"one_bit_distance_code_{which}", b.bytes(), "ok"))
    b = Bits()                                               # .. and its unused half is no code
    blk = Dynamic(b, True, lit3, [1])
    for _ in range(5):
        blk.sym(97)
    blk.sym(257); b.huff(1, 1)
    blk.sym(256)
    out.append(("one_bit_distance_code_other_half", b.bytes(), "bad"))
    b = Bits()                                               # a block without distance codes that uses one
    blk = Dynamic(b, True, lit3, [0])
    for _ in range(5):
        blk.sym(97)
    blk.sym(257); b.put(0, 16)
    out.append(("match_without_a_distance_code", b.bytes(), "bad"))
    # no end-of-block length
    simple("no_end_of_block", "bad", tail=False, lit=[8] * 256 + [0])
    # lengths 1..15 in one code, literals and distances
    lit = [0] * 286
    for i, s in enumerate([101, 32, 116, 97, 111, 110, 256, 257, 258, 264, 265, 284, 285, 0, 255, 144]):
        lit[s] = min(i + 1, 15)
    dist = [min(i + 1, 15) for i in range(16)]
    assert kraft(lit) == 32768 and kraft(dist) == 32768
    b = Bits()
    blk = Dynamic(b, True, lit, dist)
    for i in range(300):
        blk.sym((101, 32, 116, 97, 111, 110, 0, 255, 144)[rng.randrange(9) if i % 7 else i // 7 % 9])
    for di in range(16):
        for length in (3, 4, 10, 11, 12, 227, 257, 258):
            blk.match(length, DIST_BASE[di] + (1 << DIST_EXTRA[di]) - 1, top=length == 258 and di % 2 == 1)
        blk.sym(144)
    blk.sym(256)
    out.append(("lengths_1_to_15", b.bytes(), "ok"))
    # every one of the 286 literal/length symbols and the 30 distance codes has a code
    lit = [8] * 226 + [9] * 60
    dist = [4] * 2 + [5] * 28
    assert kraft(lit) == 32768 and kraft(dist) == 32768
    b = Bits()
    blk = Dynamic(b, True, lit, dist)
    for _ in range(128):
        for s in range(256):
            blk.sym(s)
    for li in range(29):
        blk.match(LEN_BASE[li], DIST_BASE[li] + (1 << DIST_EXTRA[li]) - 1)
        blk.sym(li)
    blk.match(258, 32768, top=True); blk.match(4, 1)
    blk.sym(256)
    out.append(("all_286_and_30_symbols", b.bytes(), "ok"))
    return out


def _stored_blocks(rng):
    out = []
    b = Bits(); stored(b, True, b"")
    out.append(("stored_len_0", b.bytes(), "ok"))
    b = Bits(); stored(b, True, bytes(rng.getrandbits(8) for _ in range(65535)))
    out.append(("stored_len_65535", b.bytes(), "ok"))
    for name, ln, nlen in (("one_bit", 5, 0xFFFA ^ 0x0100), ("equal", 5, 5), ("zero", 0, 0)):
        b = Bits(); stored(b, True, b"hello"[:ln], nlen=nlen)
        out.append((f"stored_nlen_{name}", b.bytes(), "bad"))
    # behind each of the eight bit offsets: empty fixed blocks (ten bits) and blocks of one nine-bit literal (nineteen)
    for r in range(8):
        j, m = next((j, m) for m in range(2) for j in range(8) if (10 * j + 19 * m + 3) % 8 == r)
        b = Bits()
        for _ in range(j):
            Fixed(b, False).sym(256)
        for _ in range(m):
            blk = Fixed(b, False); blk.sym(200); blk.sym(256)
        assert (b.n + 3) % 8 == r
        stored(b, False, bytes(rng.getrandbits(8) for _ in range(70)))
        blk = Fixed(b, True); blk.sym(33); blk.sym(256)
        out.append((f"stored_behind_bit_offset_{r}", b.bytes(), "ok"))
    b = Bits(); stored(b, True, b"0123456789")
    out.append(("stored_len_past_the_input", b.bytes()[:-1], "bad"))
    b = Bits(); b.put(1, 1); b.put(0, 2); b.align(); b.put(10, 16)
    out.append(("stored_header_cut", b.bytes(), "bad"))
    for final in (0, 1):
        b = Bits(); b.put(final, 1); b.put(3, 2); b.put(0, 61)
        out.append((f"btype_3_final_{final}", b.bytes(), "bad"))
    return out


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """[(name, raw stream, "ok" or "bad", zlib's bytes or None)]"""
    rng = random.Random(1951)
    cases = []
    for make in (_length_distance_walk, _overlapping_copies, _distance_limits, _fixed_block, _dynamic_header, _stored_blocks):
        cases += make(rng)
    out = []
    for name, raw, meant in cases:
        v, data = verdict(raw, ROOMY)
        assert v == meant, (NOT_MEANT, name, v)
        if meant == "bad":
            assert verdict(raw, CAP)[0] == "bad", (NOT_MEANT, name)
        out.append((name, raw, meant, data))
    assert len({c[0] for c in out}) == len(out)
    return out


# ---- damaged streams ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mutation_bases():
    bases = []
    for name in ("grammar.lsp", "xargs.1", "fields.c"):
        data = corpus(name)[:3000]
        for level in (1, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
                co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
                bases.append(co.compress(data) + co.flush())
    rng = random.Random(2000)
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    bases.append(co.compress(bytes(rng.choice(b"ab") for _ in range(2000))) + co.flush())
    return bases


@functools.lru_cache(maxsize=None)
def mutations(n, seed):
    """[(raw stream, "ok" / "bad" / "big" under CAP, zlib's bytes or None)]: n damaged streams"""
    bases = mutation_bases()
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = bytearray(rng.choice(bases))
        kind = rng.randrange(4)
        if kind == 0:
            s[rng.randrange(min(80, len(s)))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        elif kind == 2:
            for _ in range(rng.randint(1, 3)):
                s[rng.randrange(min(120, len(s)))] = rng.getrandbits(8)
        else:
            s = s[: rng.randrange(len(s))] + bytes(rng.getrandbits(8) for _ in range(rng.randrange(8)))
        raw = bytes(s)
        v, data = verdict(raw, CAP)
        out.append((raw, v, data))
    count = {v: sum(1 for c in out if c[1] == v) for v in ("ok", "bad", "big")}
    # the list is worth its time only while both verdicts are well represented and nearly nothing outgrows the destination
    assert count["big"] * 100 <= n, count
    assert count["ok"] * 5 >= n and count["bad"] * 5 >= n, count
    return out


def verdict_counts(cases, at):
    return {v: sum(1 for c in cases if c[at] == v) for v in ("ok", "bad", "big")}


# ---- packet-mode streams written by zlib -------------------------------------------------------------------------------------
def foreign_packets(data, P, level, strategy, window=32768):
    """(zlib stream, index, data): `data` in packets of P bytes, each written by its own zlib.compressobj that has the `window`
    bytes (32 KiB) in front of the packet as its dictionary -- so matches reach in front of the packet, at any distance -- and closed
    by the one-byte stored block in place of the sync flush's empty one. Index: offsets from the first DEFLATE byte."""
    assert data
    npk = (len(data) + P - 1) // P
    index, body = [0], bytearray()
    for k in range(npk):
        kw = {"zdict": data[max(0, k * P - window): k * P]} if k else {}
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, **kw)
        if k + 1 < npk:
            s = co.compress(data[k * P: (k + 1) * P - 1]) + co.flush(zlib.Z_SYNC_FLUSH)
            assert s[-4:] == b"\x00\x00\xff\xff"
            s = s[:-4] + b"\x01\x00\xfe\xff" + data[(k + 1) * P - 1: (k + 1) * P]
        else:
            s = co.compress(data[k * P:]) + co.flush(zlib.Z_FINISH)
        body += s
        index.append(len(body))
    stream = b"\x78\x01" + bytes(body) + zlib.adler32(data).to_bytes(4, "big")
    assert zlib.decompress(stream) == data
    return stream, index, data


FOREIGN_FAMILIES = ["zeros", "ab", "period", "longperiod", "runs", "alice29", "kennedy", "random"]
FOREIGN_SHAPES = [(1000, 9, zlib.Z_DEFAULT_STRATEGY), (1000, 9, zlib.Z_RLE), (1000, 9, zlib.Z_FIXED),
                  (4096, 9, zlib.Z_DEFAULT_STRATEGY), (32768, 9, zlib.Z_DEFAULT_STRATEGY)]


def expects_pending(family, strategy):
    """must phase 1 leave pending bytes on this stream? Random bytes have no matches. Z_RLE writes matches of distance 1 only, so
    a packet has a pending byte only where it begins with a repeat of the byte in front of it: sure for zeros and for the long
    runs, not for the others. Every other stream repeats what the 32 KiB in front of each packet hold."""
    if family == "random":
        return False
    return strategy != zlib.Z_RLE or family in ("zeros", "runs")


def expects_chains(family, P, strategy):
    """must the pointer jumping take more than one round? A chain ends at a byte that is final in its packet, and every packet's
    closing byte is one (it is stored): the zeros' matches have distance 1, so each pending byte points at the closing byte in
    front of its packet and one round settles it. A match of the periodic inputs reaches one period back, past the closing byte
    into bytes that are pending themselves, packet after packet: chains of many links, at P = 1000 through up to 90 packets."""
    return family in ("period", "longperiod") and P == 1000 and strategy != zlib.Z_RLE


@functools.lru_cache(maxsize=None)
def foreign_data(family, n):
    from conftest import synth
    if family == "alice29":
        return corpus("alice29.txt")[:n]
    if family == "kennedy":
        return corpus("kennedy.xls")[:n]
    return synth(family, n, 7)


@functools.lru_cache(maxsize=None)
def foreign_streams(family):
    """[(P, strategy, stream, index, data)] of one family: 90,000 bytes at P = 1000 (90 packets), 150,000 at the larger sizes"""
    return [(P, strategy) + foreign_packets(foreign_data(family, 90000 if P == 1000 else 150000), P, level, strategy)
            for P, level, strategy in FOREIGN_SHAPES]


def front_of_stream(P=1000, packets=3):
    """(zlib stream, index): packets of fixed-Huffman literals, but the first match of packet 0 -- at position 10, distance 11 --
    reaches one byte in front of the stream. Not a valid stream: zlib refuses it."""
    rng = random.Random(11)
    b = Bits()
    index = [0]
    for k in range(packets):
        blk = Fixed(b, False)
        n = 0
        if k == 0:
            for _ in range(10):
                blk.sym(rng.getrandbits(8))
            blk.match(258, 11)
            n = 268
        for _ in range(P - 1 - n):
            blk.sym(rng.getrandbits(8))
        blk.sym(256)
        stored(b, k == packets - 1, bytes([rng.getrandbits(8)]))
        index.append(b.nbytes())
    raw = b.bytes()
    assert verdict(raw, ROOMY)[0] == "bad", NOT_MEANT
    return b"\x78\x01" + raw + b"\x00\x00\x00\x01", index
