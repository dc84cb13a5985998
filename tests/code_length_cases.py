"""Histograms for the code construction of levels 2..6 (tests/test_gpu_code_lengths.py, tests/test_code_lengths_cpu.py): the
three alphabets of a dynamic block with the limits the encoder builds them under, and count vectors chosen so that the limit
bites -- which no input of the end-to-end suite makes the 15-bit limit do. Deterministic, nothing read from disk.

A case is (name, n, maxlen, freqs). CAP is what one packet can produce: 32,768 records and the end-of-block symbol, one
distance per match of three bytes or more, 286 + 30 lengths for the code-length alphabet. The Fibonacci chains F(1)..F(k) are
listed for k = 16..21 on the two large alphabets and k = 8..12 on the code-length alphabet (FIB_K); those whose sum alone is over
their alphabet's cap (k >= 19 on the distance alphabet, k = 12 on the code-length alphabet) are kept -- the routines' own bound is a
count below 2^22 -- and named in OVER_CAP.

The 300 random histograms are of two kinds, counted apart by the guards: 190 plain log-uniform draws ("random<t>": dense ones
over a third of the alphabet or more, and on the two large alphabets sparse ones over 24..48 symbols, 24..30 on the distance alphabet), of which those on the
code-length alphabet bite often, the sparse ones on the literal/length alphabet now and then and those on the distance alphabet
never; and 110 draws lifted into chains by construction ("random_chain<t>"), which always bite.
"""
import math
import random

LIMIT = {286: 15, 30: 15, 19: 7}
CAP = {286: 32769, 30: 10923, 19: 316}
FIB_K = {286: range(16, 22), 30: range(16, 22), 19: range(8, 13)}
TIE_M = {286: [2, 3, 4, 5, 63, 64, 65, 128, 255, 256, 257, 285, 286], 30: [2, 3, 4, 5, 15, 29, 30], 19: [2, 3, 4, 5, 10, 18, 19]}
RANDOM = {286: 60, 30: 30, 19: 100}            # 300 random histograms in all: plain log-uniform draws ...
RANDOM_CHAINS = {286: 60, 30: 50, 19: 0}       # ... and draws lifted to chains (random_chain_cases)
MAX_COUNT = 1 << 22                            # the heap key is count << 10 | tree index, the root's count (the sum) included
MAX_SUM = 1 << 20                              # what zz_debug_code_lengths admits: a margin below that, far above every CAP


def fib(k):
    """F(1) .. F(k) = 1, 1, 2, 3, 5, ..."""
    out = [1, 1]
    while len(out) < k:
        out.append(out[-1] + out[-2])
    return out[:k]


def _place(n, idx, counts, fill=0):
    f = [fill] * n
    for i, c in zip(idx, counts):
        f[i] = c
    return f


def _placements(n, k):
    """(tag, symbols in the order the chain's counts go to them): symbol 0 the rarest, the most frequent, outside the chain (absent,
    or with fill 1 one of the crowd of count 1 -- tied with the chain's rarest)"""
    scat = [i * (n - 1) // (k - 1) for i in range(k)]                   # 0 .. n-1, evenly
    scat1 = [1 + i * (n - 2) // (k - 1) for i in range(k)]              # 1 .. n-1: symbol 0 stays out
    return [("bottom_sym0_rarest", list(range(k))),
            ("bottom_sym0_heaviest", list(range(k - 1, -1, -1))),
            ("top_sym0_outside", list(range(n - k, n))),
            ("scattered_sym0_rarest", scat),
            ("scattered_sym0_heaviest", scat[::-1]),
            ("scattered_sym0_outside", scat1[::-1])]


def fibonacci_cases(n):
    out = []
    for k in FIB_K[n]:
        for tag, idx in _placements(n, k):
            for fill in (0, 1):                                          # fill 1: the floor merges the rest into ties
                out.append((f"fib{k}_{tag}_fill{fill}", n, LIMIT[n], _place(n, idx, fib(k), fill)))
    return out


def scaled_fibonacci_cases(n):
    """s F(1) .. s F(k): a floor of up to s changes nothing, and one just above s leaves the chain a chain -- the histograms that
    take the limiter's retry loop furthest (a plain chain gives way at a floor of 2: 1, 1, 2 become three equal counts)."""
    out = []
    for k in FIB_K[n]:
        for s in range(2, 8):
            if s * sum(fib(k)) > CAP[n]:
                continue
            chain = [s * x for x in fib(k)]
            for tag, idx in _placements(n, k):
                out.append((f"fib{k}x{s}_{tag}", n, LIMIT[n], _place(n, idx, chain)))
            if n > 2 * k:                                                # and over a crowd of count 1 that the floor lifts with it
                out.append((f"fib{k}x{s}_top_crowd", n, LIMIT[n], _place(n, list(range(k)) + list(range(n - k, n)), [1] * k + chain)))
    return out


def geometric_cases(n):
    out = []
    cap = CAP[n]
    for r in (2, 3):
        chain = [1]
        while sum(chain) + chain[-1] * r <= cap:
            chain.append(chain[-1] * r)
        k = len(chain)
        if k <= n:
            out.append((f"geo{r}_bottom", n, LIMIT[n], _place(n, range(k), chain)))
            out.append((f"geo{r}_top_reversed", n, LIMIT[n], _place(n, range(n - 1, n - 1 - k, -1), chain)))
            out.append((f"geo{r}_bottom_fill1", n, LIMIT[n], _place(n, range(k - 1), chain[:-1], 1)))
            two = [1] + chain[:-1] if sum(chain) + 1 > cap else [1] + chain   # 1, 1, r, r^2, ...: one level deeper
            if len(two) <= n:
                out.append((f"geo{r}_doubled_first", n, LIMIT[n], _place(n, range(len(two)), two)))
        # a chain and one giant symbol that takes the rest of the cap
        short = chain[: max(2, k - 3)]
        giant = cap - sum(short)
        out.append((f"geo{r}_giant_last", n, LIMIT[n], _place(n, list(range(len(short))) + [n - 1], short + [giant])))
        out.append((f"geo{r}_giant_sym0", n, LIMIT[n], _place(n, list(range(1, len(short) + 1)) + [0], short + [giant])))
    for k in list(FIB_K[n])[2:5]:                                        # the same with a Fibonacci chain under the giant
        chain = fib(k)
        if sum(chain) < cap and k + 1 <= n:
            out.append((f"fib{k}_giant_mid", n, LIMIT[n], _place(n, list(range(k)) + [n // 2], chain + [cap - sum(chain)])))
    return out


def tie_cases(n):
    out = []
    cap = CAP[n]
    for m in TIE_M[n]:
        big = cap // m
        for tag, idx in (("bottom", list(range(m))), ("top", list(range(n - m, n)))):
            if tag == "top" and m == n:
                continue
            out.append((f"tie{m}_{tag}_ones", n, LIMIT[n], _place(n, idx, [1] * m)))
            out.append((f"tie{m}_{tag}_cap", n, LIMIT[n], _place(n, idx, [big] * m)))
            lo = max(1, big // 3)
            # two distinct counts: halves (runs of equal lengths that cross the wave's 64-symbol blocks), then alternating
            out.append((f"tie{m}_{tag}_halves", n, LIMIT[n], _place(n, idx, [lo] * (m // 2) + [big] * (m - m // 2))))
            out.append((f"tie{m}_{tag}_alternating", n, LIMIT[n], _place(n, idx, [1 if i & 1 else 2 for i in range(m)])))
    return out


def degenerate_cases(n):
    L = LIMIT[n]
    out = [("all_zero", n, L, [0] * n)]
    for tag, i in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        out.append((f"one_symbol_{tag}", n, L, _place(n, [i], [7])))
    out.append(("two_symbols_ends", n, L, _place(n, [0, n - 1], [1, CAP[n] - 1])))
    out.append(("two_symbols_adjacent", n, L, _place(n, [n // 2, n // 2 + 1], [5, 5])))
    out.append(("every_symbol_once", n, L, [1] * n))
    return out


def random_cases(n):
    """log-uniform counts, clamped to the cap. The span of the counts is drawn too: the deeper ones (a few heavy symbols over a
    long tail of rare ones) are what makes a free tree deeper than the limit."""
    rng = random.Random(0xC0DE00 + n)
    cap = CAP[n]
    out = []
    for t in range(RANDOM[n]):
        if n != 19 and t & 1:                                            # sparse: few symbols, exponents up to log2 of the cap
            m = rng.randint(min(24, n - 6), min(n, 48))
            top = math.log2(cap)
        else:
            m = rng.randint(max(2, n // 3) if n != 19 else 12, n)
            top = rng.uniform(0.6, 1.0) * (cap.bit_length() - 1)         # log2 of the largest count drawn
        f = [0] * n
        for i in rng.sample(range(n), m):
            f[i] = int(2.0 ** rng.uniform(0.0, top))
        while sum(f) > cap:                                              # clamp: halve the heaviest until the packet holds them
            j = max(range(n), key=lambda i: f[i])
            f[j] = max(1, f[j] // 2)
        out.append((f"random{t}", n, LIMIT[n], f))
    return out


def random_chain_cases(n):
    """Log-uniform draws again, few of them and sorted, each lifted above the sum of those two or more below it: what a log-uniform draw almost
    never is on the two large alphabets -- a tree that stays a chain -- with random bumps in it, at random places of the alphabet
    (nothing else beside it: one more rare symbol and the two lightest merges tie, which halves the depth)."""
    rng = random.Random(0xC4A100 + n)
    cap = CAP[n]
    out = []
    while len(out) < RANDOM_CHAINS[n]:
        k = rng.randint(17, 20 if n == 286 else 18)
        c = sorted(int(2.0 ** rng.uniform(0.0, 9.0)) for _ in range(k))
        for i in range(2, k):
            c[i] = max(c[i], sum(c[:i - 1]) + 1)                         # heavier than everything two or more below it, merged
        if sum(c) > cap:
            continue
        out.append((f"random_chain{len(out)}", n, LIMIT[n], _place(n, rng.sample(range(n), k), c)))
    return out


def cases(n):
    return (fibonacci_cases(n) + scaled_fibonacci_cases(n) + geometric_cases(n) + tie_cases(n) + degenerate_cases(n) +
            random_cases(n) + random_chain_cases(n))


OVER_CAP = {n: sorted(name for name, _, _, f in fibonacci_cases(n) if sum(f) > CAP[n]) for n in (286, 30, 19)}
