"""The device code construction of levels 2..6 (zz_level2.h calc_lengths_w, generate_codes_w, rle_lengths_w; zz_level6.h
pm_lengths_w) against the oracle, on histograms where the length limit bites.

The end-to-end parity tests reach these routines only through the histograms their inputs produce, and on the literal/length and
distance alphabets none of them makes a free Huffman tree deeper than 15: there the retry loop of the frequency-floor limiter, a
biting package-merge and a floor above 1 or 2 never ran on the GPU. zz_debug_code_lengths runs the routines, as the packet kernels
instantiate them and on the same LDS layout, on histograms of the caller's: tests/code_length_cases.py. Every output is compared
exactly with the oracle's export of the same step (zzo_calc_lengths, zzo_pm_lengths, zzo_generate, zzo_from_lengths).

Cost, counted with the oracle on the CPU: a plain Fibonacci chain gives way at a floor of 2 (1, 1, 2 become three equal counts and the
chain a balanced tree), so the deepest retry loops belong to the scaled chains: 7 F(1) .. 7 F(17) on the literal/length alphabet takes
11 retries of the heap build (floor 11), 18 cases a floor of 8 or more, all cases of that alphabet 551 retries together; the distance
alphabet's worst is 4, the code-length alphabet's 3. All cases of one alphabet and mode go in one launch, a wavefront each.

The case list holds the Fibonacci chains F(1)..F(k) for k = 16..21 on the two large alphabets and k = 8..12 on the code-length
alphabet. Of these, k >= 19 sums to more than the 10,923 distances and k = 12 to more than the 316 code lengths a packet can hold: they
are kept (the routines' own bound is a count below 2^22) and listed in OVER_CAP; every other case stays within a packet's caps.

The case list is tests/code_length_cases.py; the oracle bindings, the analysis and the guards are tests/code_length_checks.py, which
tests/test_code_lengths_cpu.py runs against the oracle alone."""
import ctypes

import pytest

from code_length_checks import (ALPHABETS, ANCHORS, MODES, CodeOracle, analyse, anchor_input, blocks_over_the_code_length_limit,
                                check_guards, check_lengths)


# ---- the device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import torch
    import zzflate_amd as zz
    assert torch.cuda.is_available()
    return zz.Context(0)


def run_device(ctx, rows, mode):
    """one launch of zz_debug_code_lengths over `rows`; per case (lens, codes, records or None, meta frequencies or None)"""
    import zzflate_amd as zz
    k = len(rows)
    desc, freqs = (ctypes.c_uint32 * (4 * k))(), (ctypes.c_uint32 * (288 * k))()
    for c, r in enumerate(rows):
        desc[4 * c], desc[4 * c + 1], desc[4 * c + 2] = mode, r["n"], r["maxlen"]
        freqs[288 * c:288 * c + r["n"]] = r["f"]
    lens, codes = (ctypes.c_uint8 * (288 * k))(), (ctypes.c_uint32 * (288 * k))()
    recs, meta = (ctypes.c_uint16 * (320 * k))(), (ctypes.c_uint32 * (20 * k))()
    rc = zz.lib.zz_debug_code_lengths(ctx._h, k, desc, freqs, lens, codes, recs, meta)
    assert rc == 0, zz.lib.zz_last_error()
    out = []
    for c, r in enumerate(rows):
        n = r["n"]
        nr = meta[20 * c + 19]
        assert nr <= 320
        out.append((list(lens[288 * c:288 * c + n]), list(codes[288 * c:288 * c + n]),
                    list(recs[320 * c:320 * c + nr]) if n != 19 else None, list(meta[20 * c:20 * c + 19]) if n != 19 else None))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALPHABETS)
def test_device_code_construction_matches_the_oracle(ctx, oracle, n):
    """both builders, every case of the alphabet: lengths, canonical codes, run-length records and meta frequencies, exactly"""
    A = analyse(oracle)
    check_guards(A)
    co, rows = A["co"], A[n]
    got = {mode: run_device(ctx, rows, mode) for mode in MODES}
    bad = []
    for mode in MODES:
        for i, (r, (lens, codes, recs, meta)) in enumerate(zip(rows, got[mode])):
            want = r["want"][mode]
            if lens != want:
                bad.append((r["name"], mode, "lengths", r["f"], lens, want))
                continue
            check_lengths(r, lens, mode, got[0][i][0])
            if codes != co.generate(want):
                bad.append((r["name"], mode, "codes"))
            if n != 19 and (recs, meta) != co.from_lengths(want):
                bad.append((r["name"], mode, "records", recs, meta, co.from_lengths(want)))
    assert not bad, (len(bad), bad[:3])


@pytest.mark.gpu
def test_hook_refuses_what_the_heap_key_cannot_hold(ctx):
    import zzflate_amd as zz
    # sums to more than 2^20, the hook's margin (the heap key count << 10 | index holds a root below 2^22, a packet sums to 32,769)
    row = dict(n=30, maxlen=15, f=[1 << 20, 1] + [0] * 28)
    with pytest.raises(AssertionError):
        run_device(ctx, [row], 0)
    assert b"2^20" in zz.lib.zz_last_error()
    with pytest.raises(AssertionError):
        run_device(ctx, [dict(n=30, maxlen=7, f=[1] * 30)], 0)       # a limit the packet kernels never ask for


@pytest.mark.gpu
@pytest.mark.parametrize("name,P", ANCHORS)
def test_end_to_end_inputs_that_cross_the_code_length_retry_loop(ctx, oracle, name, P):
    """The one place the end-to-end path does reach a biting limit: the 19-symbol code-length alphabet under its 7 bits. The first
    160,000 bytes of these three inputs have blocks whose code-length histogram wants a tree of depth 8 (the walk asserts it on
    the oracle's level-2 stream), so levels 2 and 6 run the limiter's retry loop / a biting package-merge inside the encoder."""
    import torch
    import zzflate_amd as zz
    co = CodeOracle(oracle)
    d = anchor_input(name)
    src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    ctx.set_extended_levels(True)
    try:
        for lvl in (2, 6):
            want = oracle.encode_packets(d, 2, lvl, P)
            if lvl == 2:
                over, blocks = blocks_over_the_code_length_limit(co, want)
                assert over >= 1 and blocks >= 5, (name, over, blocks)
            cap = zz.bound(len(d), zz.Format.Deflate, 2, P)
            dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            w = ctx.encode(src, len(d), dst, cap, zz.Format.Deflate, lvl, P)
            assert dst[:w].cpu().numpy().tobytes() == want, (name, P, lvl)
    finally:
        ctx.set_extended_levels(False)
