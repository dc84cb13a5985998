"""What tests/test_gpu_code_lengths.py and tests/test_code_lengths_cpu.py share beside the case list (code_length_cases.py): the
oracle's Huffman exports on Python lists, the analysis of every case with the oracle (free depth, floor, retries, the lengths both
builders must give), the guards that keep the comparison from passing on histograms that ask nothing of the routines, the properties
any result must have, and a block walk that recovers the code-length histograms of a deflate stream. No GPU is needed here."""
import ctypes
import os

import code_length_cases as clc
from conftest import CORPUS
from test_oracle_extended import best_cost      # the exhaustive optimum the package-merge tests of the oracle are held to

ALPHABETS = (286, 30, 19)
MODES = (0, 1)                       # 0: frequency-floor limiter (levels 2, 3), 1: package-merge (levels 4..6)
ANCHORS = (("kennedy.xls", 32768), ("ptt5", 4096), ("sum", 4096))
ANCHOR_BYTES = 160000


class CodeOracle:
    """the oracle's Huffman exports (oracle/zzoracle.h), on Python lists"""

    def __init__(self, oracle):
        L = oracle.L
        pi, pu32, pu8 = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        L.zzo_calc_lengths.restype = None; L.zzo_calc_lengths.argtypes = [pi, ctypes.c_int, ctypes.c_int, pi]
        L.zzo_pm_lengths.restype = None; L.zzo_pm_lengths.argtypes = [pi, ctypes.c_int, ctypes.c_int, pi]
        L.zzo_generate.restype = None; L.zzo_generate.argtypes = [pi, ctypes.c_int, pi, pu32]
        L.zzo_from_lengths.restype = ctypes.c_int; L.zzo_from_lengths.argtypes = [pi, ctypes.c_int, pi, pu8, pu8]
        self.L = L

    def _lengths(self, fn, freqs, maxlen):
        n = len(freqs)
        out = (ctypes.c_int * n)()
        fn((ctypes.c_int * n)(*freqs), n, maxlen, out)
        return list(out)

    def calc(self, freqs, maxlen):
        return self._lengths(self.L.zzo_calc_lengths, freqs, maxlen)

    def pm(self, freqs, maxlen):
        return self._lengths(self.L.zzo_pm_lengths, freqs, maxlen)

    def generate(self, lens):
        """codes packed as the device packs them: (len << 16) | bits, 0 for an unused symbol"""
        n = len(lens)
        ol, ob = (ctypes.c_int * n)(), (ctypes.c_uint32 * n)()
        self.L.zzo_generate((ctypes.c_int * n)(*lens), n, ol, ob)
        return [(l << 16) | b for l, b in zip(ol, ob)]

    def from_lengths(self, lens):
        """(records packed value | payload << 8, the 19 meta frequencies they add)"""
        n = len(lens)
        f19 = (ctypes.c_int * 19)()
        val, pay = (ctypes.c_uint8 * 320)(), (ctypes.c_uint8 * 320)()
        nv = self.L.zzo_from_lengths((ctypes.c_int * n)(*lens), n, f19, val, pay)
        return [val[i] | (pay[i] << 8) for i in range(nv)], list(f19)


def floor_of(co, freqs, maxlen, limited):
    """the frequency floor CalcLengths ends on, by its own rule (huffman.cpp:122-154), and the retries it took"""
    total, floor, retries = sum(freqs), 0, 0
    while co.calc([max(f, floor) if f else 0 for f in freqs], 30) != limited:
        floor += max(1, total >> maxlen)
        retries += 1
        assert retries < 4096
    return floor, retries


_ANALYSIS = {}


def analyse(oracle):
    """per alphabet, per case: the free depth, the oracle's lengths under the limit for both modes, the floor. Computed once."""
    if not _ANALYSIS:
        co = CodeOracle(oracle)
        for n in ALPHABETS:
            rows = []
            for name, nn, maxlen, f in clc.cases(n):
                assert nn == n and len(f) == n and maxlen == clc.LIMIT[n]
                lim = co.calc(f, maxlen)
                floor, retries = floor_of(co, f, maxlen, lim)
                rows.append(dict(name=name, n=n, maxlen=maxlen, f=f, depth=max(co.calc(f, 30)), want=(lim, co.pm(f, maxlen)),
                                 floor=floor, retries=retries))
            _ANALYSIS[n] = rows
        _ANALYSIS["co"] = co
    return _ANALYSIS


def check_guards(A):
    """the case list does what it is there for: enough cases where the limit bites, deep floors, a packet's caps"""
    need = {286: 40, 30: 20, 19: 20}
    for n in ALPHABETS:
        rows = A[n]
        assert len({r["name"] for r in rows}) == len(rows)
        assert sum(r["depth"] > r["maxlen"] for r in rows) >= need[n], n
        for r in rows:
            assert all(0 <= x < clc.MAX_COUNT for x in r["f"]) and sum(r["f"]) <= clc.MAX_SUM, r["name"]
            assert sum(r["f"]) <= clc.CAP[n] or r["name"] in clc.OVER_CAP[n], r["name"]
            assert (r["floor"] > 0) == (r["depth"] > r["maxlen"]), r["name"]
    assert clc.OVER_CAP[286] == [] and all(nm.startswith(("fib19_", "fib20_", "fib21_")) for nm in clc.OVER_CAP[30])
    assert all(nm.startswith("fib12_") for nm in clc.OVER_CAP[19])
    everything = [r for n in ALPHABETS for r in A[n]]
    assert sum(r["floor"] >= 8 for r in everything) >= 10
    # the random histograms, the two kinds counted apart: the chains bite by construction (17 or more counts, each above the sum of all
    # two or more below it: a free depth of 16 or more), the plain draws only where the draw happens to -- often on the code-length
    # alphabet, now and then on the literal/length alphabet
    chains = [r for r in everything if r["name"].startswith("random_chain")]
    plain = [r for r in everything if r["name"].startswith("random") and r not in chains]
    bite = lambda rows: sum(r["depth"] > r["maxlen"] for r in rows)
    assert len(plain) == 190 and len(chains) == 110
    assert bite(chains) == 110 and all(r["n"] != 19 for r in chains)
    assert bite(plain) >= 40 and bite([r for r in plain if r["n"] != 19]) >= 1
    assert bite(plain) + bite(chains) >= 100


def cost(f, lens):
    return sum(x * l for x, l in zip(f, lens))


def check_lengths(r, lens, mode, other=None):
    """what any result of the limiter (mode 0) or of package-merge (mode 1) must satisfy; `other`: mode 0's lengths of the same case"""
    f, maxlen = r["f"], r["maxlen"]
    tag = (r["name"], r["n"], mode)
    assert max(lens) <= maxlen, tag
    assert sum(1 << (maxlen - l) for l in lens if l) <= 1 << maxlen, tag                    # Kraft, in units of 2^-maxlen
    assert all((l > 0) == (x > 0) for l, x in zip(lens, f)), tag
    if mode == 1:
        assert cost(f, lens) <= cost(f, other), tag
        used = [x for x in f if x]
        if 2 <= len(used) <= 14 and maxlen <= 7:
            assert cost(f, lens) == best_cost(f, maxlen), tag


# ---- a block walk: the code-length histogram of every dynamic header of a raw deflate stream ------------------------------------
_LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DEXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _table(lens):
    """peeked bits (LSB first) -> (symbol, length), for a canonical code"""
    mx = max(lens) if any(lens) else 1
    count = [0] * (mx + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, c = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    tab = [None] * (1 << mx)
    for s, l in enumerate(lens):
        if l:
            code = nxt[l]; nxt[l] += 1
            rev = int(format(code, "0%db" % l)[::-1], 2)
            for k in range(rev, 1 << mx, 1 << l):
                tab[k] = (s, l)
    return tab, mx


def walk_code_length_histograms(raw):
    """A small inflate over a raw deflate stream that keeps no output: per dynamic block, the counts of the 19 code-length symbols
    its header spends on the literal/length and distance lengths -- the histogram the encoder built its code-length code from."""
    data = raw + bytes(8)
    pos = 0                                      # in bits

    def bits(k):
        nonlocal pos
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << k) - 1)
        pos += k
        return v

    def sym(tab, mx):
        nonlocal pos
        s, l = tab[(int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << mx) - 1)]
        pos += l
        return s

    out = []
    while True:
        final, kind = bits(1), bits(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF
            pos += 8 * n
        else:
            assert kind in (1, 2)
            if kind == 1:
                lit, dist = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = bits(3)
                ctab, cmx = _table(cl)
                hist, lens = [0] * 19, []
                while len(lens) < hlit + hdist:
                    s = sym(ctab, cmx)
                    hist[s] += 1
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
                assert len(lens) == hlit + hdist
                lit, dist = lens[:hlit], lens[hlit:]
                out.append(hist)
            ltab, lmx = _table(lit)
            dtab, dmx = _table(dist)
            while True:
                s = sym(ltab, lmx)
                if s == 256:
                    break
                if s > 256:
                    pos += _LEXTRA[s - 257]
                    d = sym(dtab, dmx)                   # (advances pos itself: not inside an augmented assignment to it)
                    pos += _DEXTRA[d]
        if final:
            assert (pos + 7) >> 3 == len(raw)
            return out


def anchor_input(name):
    return open(os.path.join(CORPUS, name), "rb").read()[:ANCHOR_BYTES]


def blocks_over_the_code_length_limit(co, stream):
    """(dynamic blocks whose code-length histogram wants a tree deeper than 7, dynamic blocks) of a raw deflate stream"""
    hists = walk_code_length_histograms(stream)
    return sum(max(co.calc(h, 30)) > 7 for h in hists), len(hists)
