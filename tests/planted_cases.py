"""Planted-match inputs for the encoders' internal boundaries (tests/test_planted_cases_cpu.py, tests/test_gpu_planted.py).
Deterministic, nothing read from disk, no torch.

The background is a de Bruijn sequence B(40, 3) -- 64,000 symbols, every trigram exactly once -- mapped through a fixed permutation
of the byte values: it holds no match of three bytes or more, so every match an encoder finds in a case is one that was planted
(or a chance extension of it by a byte or two), and with 40 symbols it still compresses at levels 2 and above, so no block falls
back to stored. 15 of the 40 byte values are above 143: a good third of the bytes take 9-bit codes in a fixed block.

A case is (family, boundary, p, L, D) or (family, boundary, p, L, D, (p2, L2, D2)): the background cut to N bytes, then bytes
[p, p + L) set to a copy from distance D, byte by byte, so that the copy overlaps itself where D < L. A case with p - D < 0 or
p + L > N is dropped. The `lazy` family carries a second copy, 40 bytes at p + 1 from distance 1500 behind the 6 bytes at p from
distance 500: for both to stand, the far source's first five bytes are first made equal to the near source's (plant()), an echo
1000 bytes apart and 499 bytes in front of p. The `backcap` family (not in the issue's list; added because no other family moves
the 258-byte cap on backward extension) is a run of period 259 or more across the packet edge.

Geometry A is two packets of 32,768 bytes, the second cut at 20,000; geometry B is three packets of P = 4096, 1000 or 777 bytes and
500 bytes of a fourth. The boundaries are where the encoders change what they do: the 64-position blocks the parsers alternate over,
the 16,384-byte batch switch of levels 2 and 3, target = n - 258 of a packet, the packet edge, and the same again in the second packet.
"""

SYMBOLS = 40
A_P, A_N = 32768, 32768 + 20000
A_BOUNDS = [64, 16384, 32768 - 258, 32768, 32768 + 64, 32768 + 16384, A_N - 258]
B_PACKETS = [4096, 1000, 777]
POS_LD = [(9, 1000), (258, 1000), (300, 3)]
NEAR = 50
LEN_L = [3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 258, 259, 300, 600]
LEN_D = 777
DIST_D = [1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769]
DIST_L = 40
LAZY_BOUNDS = [64, 16384, 32768 + 64]           # (at 64 every case is dropped: 1500 bytes in front of p do not exist there)
LAZY = (6, 500, 40, 1500)
RUN_BOUNDS = [16384, 32768]                     # `backcap`: a run of period D >= 259 across the batch switch and the packet edge
RUN_D = [259, 300, 517]


def de_bruijn(k, n):
    """B(k, n) in the order of Fredricksen, Kessler and Maiorana: the Lyndon words over k symbols whose length divides n, in
    lexicographic order (Duval's iteration, no recursion)."""
    seq, w = [], [-1]
    while w:
        w[-1] += 1
        m = len(w)
        if n % m == 0:
            seq.extend(w)
        while len(w) < n:
            w.append(w[-m])
        while w and w[-1] == k - 1:
            w.pop()
    return seq


def permutation(seed):
    """a Fisher-Yates shuffle of 0..255 driven by a 64-bit linear congruential generator: the same on every Python"""
    perm = list(range(256))
    x = seed
    for i in range(255, 0, -1):
        x = (x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        j = (x >> 33) % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def _background():
    perm = permutation(3)
    return bytes(perm[s] for s in de_bruijn(SYMBOLS, 3))


BACKGROUND = _background()


def geometry_b(P):
    """(N, boundaries) of three packets of P bytes and 500 more"""
    n = 3 * P + 500
    b = set()
    for k in range(4):
        b.update((k * P + 64, k * P + P - 258, (k + 1) * P))
    b.add(n - 258)
    return n, sorted(x for x in b if 0 < x <= n)


def _keep(n, out, case):
    copies = [case[2:5]] + ([case[5]] if len(case) > 5 else [])
    if all(p - d >= 0 and p + l <= n and p >= 0 for p, l, d in copies) and case not in out[1]:
        out[0].append(case)
        out[1].add(case)


def pos_cases(n, bounds, far=1000):
    """`far` stands in for 1000 where packets are shorter than that; at a boundary that not even `far` bytes lie in front of
    (64, the first block's end) the distance is NEAR, so that the boundary is crossed by more than the run of distance 3"""
    out = ([], set())
    for b in bounds:
        for l, d in POS_LD:
            for p in range(b - 70, b + 71):
                _keep(n, out, ("pos", b, p, l, (far if b >= far else NEAR) if d == 1000 else d))
    return out[0]


def len_cases(n, bounds):
    out = ([], set())
    for b in bounds:
        for l in LEN_L:
            for p in (b - l // 2, b - l, b):
                _keep(n, out, ("len", b, p, l, LEN_D))
    return out[0]


def dist_cases(n, bounds):
    out = ([], set())
    for b in bounds:
        for d in DIST_D:
            for p in (b - 20, b + 1):
                _keep(n, out, ("dist", b, p, DIST_L, d))
    return out[0]


def start_cases(n):
    out = ([], set())
    for p in range(1, 81):
        for d in (1, 2, 3, 8, p):
            for l in (9, 40):
                _keep(n, out, ("start", 0, p, l, d))
    return out[0]


def start_far_cases(n, P):
    out = ([], set())
    for p in (P + 1, P + 64, P + 300):
        for s in range(10):
            _keep(n, out, ("start-far", P, p, 40, p - s))
    return out[0]


def lazy_cases(n, bounds=LAZY_BOUNDS):
    l1, d1, l2, d2 = LAZY
    out = ([], set())
    for b in bounds:
        for p in range(b - 70, b + 71):
            _keep(n, out, ("lazy", b, p, l1, d1, (p + 1, l2, d2)))
    return out[0]


def backcap_cases(n, bounds=RUN_BOUNDS):
    """a run of period D that starts k bytes in front of the boundary and goes on for a period and 60 bytes behind it: a cold
    packet sees no candidate in its first D bytes, so the match found behind them has more than 258 bytes to extend backward
    over (the cap of defect D11, oracle/zzoracle.c)"""
    out = ([], set())
    for b in bounds:
        for d in RUN_D:
            for k in (0, 1, 40, d):
                _keep(n, out, ("backcap", b, b - k, k + d + 60, d))
    return out[0]


def cases_a():
    """geometry A: every family"""
    return (pos_cases(A_N, A_BOUNDS) + len_cases(A_N, A_BOUNDS) + dist_cases(A_N, A_BOUNDS) + start_cases(A_N) + lazy_cases(A_N) +
            backcap_cases(A_N))


def cases_b(P):
    """geometry B: `pos` for every mode; `dist` and `start-far` for the warm window"""
    n, bounds = geometry_b(P)
    return pos_cases(n, bounds, 1000 if P >= 1000 + 70 else 300) + dist_cases(n, bounds) + start_far_cases(n, P)


def size_of(geometry):
    """geometry is "A" or a packet size of geometry B: (P, N)"""
    return (A_P, A_N) if geometry == "A" else (geometry, geometry_b(geometry)[0])


def plant(case, n):
    """the case's input"""
    b = bytearray(BACKGROUND[:n])
    copies = [case[2:5]]
    if len(case) > 5:
        p, l, d = case[2:5]
        d2 = case[5][2]
        assert case[5][0] == p + 1 and d2 > d
        copies = [(p + 1 - d, l - 1, d2 - d), case[2:5], case[5]]       # the echo: 5 bytes at p - 499 from distance 1000
    for p, l, d in copies:
        if d >= l:
            b[p:p + l] = b[p - d:p - d + l]
        else:
            for i in range(p, p + l):
                b[i] = b[i - d]
    return bytes(b)


def cells(cases):
    """the cases by (family, boundary), in first-seen order: what one GPU test runs"""
    out = {}
    for c in cases:
        out.setdefault((c[0], c[1]), []).append(c)
    return out


# the modes of both test files: (level, warm window); levels 4..6 bring their own window
MODES = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (1, 258), (1, 32768), (2, 4096), (3, 32768)]
