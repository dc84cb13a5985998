"""wg_scan_excl / wg_scan_excl2 (zz_wave.h), the workgroup prefix sum of every planning kernel, alone: zz_debug_wg_scan runs one
workgroup of T threads over n values as the kernels do -- one value per thread and round, a carry between rounds -- and hands
back the exclusive prefixes and the total. The yardstick is numpy.cumsum in the form's width. The sizes sit on the edges of a
wavefront (63, 64, 65) and of a round (T - 1, T, T + 1, 2T + 1). Needs a real MI355X: run with `-m gpu`."""
import ctypes

import numpy as np
import pytest

import zzflate_amd as zz

pytestmark = pytest.mark.gpu
U32, U64, PAIR = 0, 1, 2
THREADS = [256, 1024]


def sizes(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    return zz.Context(0)


def scan(ctx, form, T, values):
    """(exclusive prefixes, total) of one call; `values` is the form's array (PAIR: shape (n, 2) of uint64)"""
    values = np.ascontiguousarray(values)
    out = np.full_like(values, 0x55)
    total = np.full(values.shape[1:] or (1,), 0x55, dtype=values.dtype)
    rc = zz.lib.zz_debug_wg_scan(ctx._h, form, T, values.shape[0], values.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                 total.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, zz.lib.zz_last_error()
    return out, total


def exclusive(values):
    """cumsum in the array's own width (numpy wraps unsigned sums), shifted by one; and the sum of all"""
    incl = np.cumsum(values, axis=0, dtype=values.dtype)
    excl = np.concatenate([np.zeros_like(values[:1]), incl[:-1]]) if len(values) else incl
    return excl, (incl[-1] if len(values) else np.zeros(values.shape[1:], dtype=values.dtype))


@pytest.mark.parametrize("T", THREADS)
def test_u32_sums_wrap(ctx, T):
    rng = np.random.default_rng(T)
    for n in sizes(T):
        # values of 2^30 and more: the running sum passes 2^32 within every four elements
        v = rng.integers(1 << 30, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        want, want_total = exclusive(v)
        if n >= 4:
            assert int(v.astype(np.uint64).sum()) >= 1 << 32 and want.dtype == np.uint32
        got, total = scan(ctx, U32, T, v)
        assert got.dtype == np.uint32 and np.array_equal(got, want), n
        assert int(total[0]) == int(want_total), n


@pytest.mark.parametrize("T", THREADS)
def test_u64(ctx, T):
    rng = np.random.default_rng(T + 1)
    for n in sizes(T):
        v = rng.integers((1 << 40) - 1000, (1 << 40) + 1000, size=n, dtype=np.uint64)
        want, want_total = exclusive(v)
        got, total = scan(ctx, U64, T, v)
        assert np.array_equal(got, want), n
        assert int(total[0]) == int(want_total) and (n == 0 or int(want_total) >= n << 39), n


@pytest.mark.parametrize("T", THREADS)
def test_pair_of_u32_and_u64_between_one_pair_of_barriers(ctx, T):
    rng = np.random.default_rng(T + 2)
    for n in sizes(T):
        a = rng.integers(1 << 30, 1 << 32, size=n, dtype=np.uint64)
        b = rng.integers((1 << 40) - 1000, (1 << 40) + 1000, size=n, dtype=np.uint64)
        want_a, total_a = exclusive(a.astype(np.uint32))
        want_b, total_b = exclusive(b)
        got, total = scan(ctx, PAIR, T, np.stack([a, b], axis=1).reshape(n, 2))
        assert np.array_equal(got[:, 0], want_a.astype(np.uint64)), n          # (the 32-bit sums come back zero-extended)
        assert np.array_equal(got[:, 1], want_b), n
        assert (int(total[0]), int(total[1])) == (int(total_a), int(total_b)), n


def test_refusals(ctx):
    v = np.zeros(4, dtype=np.uint64)
    p = v.ctypes.data_as(ctypes.c_void_p)
    assert zz.lib.zz_debug_wg_scan(ctx._h, 3, 256, 4, p, p, p) == zz.E_ARG
    assert zz.lib.zz_debug_wg_scan(ctx._h, U64, 512, 4, p, p, p) == zz.E_ARG
    assert zz.lib.zz_debug_wg_scan(ctx._h, U64, 256, 4, None, p, p) == zz.E_ARG
    assert zz.lib.zz_debug_wg_scan(None, U64, 256, 4, p, p, p) == zz.E_ARG
