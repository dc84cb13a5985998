"""The inflate core's verdict against zlib's, on the CPU: every stream of tests/deflate_cases.py -- hand-made boundary streams,
damaged zlib streams, packet-mode streams written by zlib -- through tests/cxx/inflate_harness.cpp and inflate_items_harness.cpp
built with g++ -DZZ_INFLATE_CHECKED (every buffer access of the core bounds-checked; out of range aborts). Raw DEFLATE has no
checksum, so only the block rules stand between a damaged stream and wrong bytes: a stream zlib decodes gives exactly zlib's
bytes, one zlib refuses gives E_DATA, one that outgrows the destination E_DATA or E_NOSPACE. test_gpu_decode_conformance.py
sends the same streams (same generator, same seeds) to the device: each has first passed a bounds-checked run here."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from deflate_cases import (CAP, FOREIGN_FAMILIES, boundary_cases, expects_chains, expects_pending, foreign_streams, front_of_stream,
                           mutations, verdict_counts)

import zzflate_amd as zz

u64 = ctypes.c_uint64
GUARD = 64
N_MUTATIONS, SEED = 20000, 1


def build(tmp, name):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the inflate harnesses")
    so = str(tmp / f"lib{name}.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-DZZ_INFLATE_CHECKED",
                    "-o", so, os.path.join(ROOT, "tests", "cxx", name + ".cpp")], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    L = build(tmp_path_factory.mktemp("conformance"), "inflate_harness")
    L.zih_inflate.restype = ctypes.c_int
    L.zih_inflate.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.POINTER(u64)]
    L.zih_packets.restype = ctypes.c_int
    L.zih_packets.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(u64), u64, ctypes.c_void_p, u64,
                              ctypes.POINTER(u64), ctypes.POINTER(u64)]
    return L


@pytest.fixture(scope="module")
def T(tmp_path_factory):
    L = build(tmp_path_factory.mktemp("conformance_items"), "inflate_items_harness")
    L.zit_item.restype = ctypes.c_int
    L.zit_item.argtypes = [ctypes.c_char_p, u64, ctypes.c_int, ctypes.c_void_p, u64, ctypes.c_uint32, ctypes.POINTER(u64)]
    return L


def inflate(H, s, fmt, cap):
    out = ctypes.create_string_buffer(max(cap, 1))
    n = u64(0)
    rc = H.zih_inflate(s, len(s), fmt, out, cap, ctypes.byref(n))
    return rc, out.raw[: n.value]


def packets(H, s, fmt, P, index, cap):
    idx = (u64 * len(index))(*index)
    out = ctypes.create_string_buffer(max(cap, 1))
    n = u64(0)
    stats = (u64 * 3)()
    rc = H.zih_packets(s, len(s), fmt, P, idx, len(index), out, cap, ctypes.byref(n), stats)
    return rc, out.raw[: n.value], list(stats)


def item(T, s, cap, lanes):
    """(status, decoded bytes) of the raw stream `s`; the GUARD bytes behind `cap` must come back untouched"""
    out = ctypes.create_string_buffer(b"\xEE" * (cap + GUARD), cap + GUARD)
    n = u64(0)
    rc = T.zit_item(s, len(s), 2, out, cap, lanes, ctypes.byref(n))
    assert rc != -100, "the simulated lanes disagree"
    assert out.raw[cap:] == b"\xEE" * GUARD, "bytes behind the destination's capacity were written"
    assert rc == 0 or n.value == 0
    return rc, out.raw[: n.value]


def check(got, v, data, what):
    """the exact rule: zlib's bytes, or E_DATA; a stream that outgrows the destination may be refused either way"""
    rc, out = got
    if v == "ok":
        assert rc == 0 and out == data, (what, rc, len(out), len(data))
    elif v == "bad":
        assert rc == zz.E_DATA, (what, rc)
    else:
        assert rc in (zz.E_DATA, zz.E_NOSPACE), (what, rc)


def cap_of(v, data):
    return len(data) if v == "ok" else CAP


BOUNDARY = boundary_cases()


@pytest.mark.parametrize("name,raw,v,data", BOUNDARY, ids=[c[0] for c in BOUNDARY])
def test_boundary_cases(H, T, name, raw, v, data):
    cap = cap_of(v, data)
    check(inflate(H, raw, 2, cap), v, data, name)
    check(inflate(H, raw, 2, cap + 100), v, data, name)
    for lanes in (1, 64):
        check(item(T, raw, cap, lanes), v, data, (name, lanes))
    if v == "ok" and data:
        assert inflate(H, raw, 2, cap - 1)[0] == zz.E_NOSPACE, name
        assert item(T, raw, cap - 1, 64)[0] == zz.E_NOSPACE, name


def test_mutations(H, T):
    cases = mutations(N_MUTATIONS, SEED)
    print("mutations per verdict:", verdict_counts(cases, 1))
    for i, (raw, v, data) in enumerate(cases):
        cap = cap_of(v, data)
        check(inflate(H, raw, 2, cap), v, data, i)
        check(item(T, raw, cap, 1), v, data, i)
        if i % 16 == 0:
            check(item(T, raw, cap, 64), v, data, (i, 64))


@pytest.mark.parametrize("family", FOREIGN_FAMILIES)
def test_foreign_packet_streams(H, family):
    for P, strategy, s, idx, data in foreign_streams(family):
        assert inflate(H, s, 0, len(data)) == (0, data), (P, strategy)
        rc, out, stats = packets(H, s, 0, P, idx, len(data))
        print(f"{family} P={P} strategy={strategy}: pending {stats[0]}, rounds {stats[1]}, packets with pending bytes {stats[2]}")
        assert (rc, out) == (0, data), (P, strategy)
        if expects_pending(family, strategy):
            assert stats[0] > 0, "expected matches that reach in front of a packet's start"
        if expects_chains(family, P, strategy):
            assert stats[1] > 1, "expected chains of more than one link"
        # a lying index: an error or the exact bytes
        for j in (1, len(idx) // 2, len(idx) - 2):
            for d in (-1, 1):
                bad = list(idx); bad[j] += d
                rc, out, _ = packets(H, s, 0, P, bad, len(data))
                assert rc != 0 or out == data, (P, j, d)


def test_first_match_in_front_of_the_stream(H):
    s, idx = front_of_stream()
    assert inflate(H, s, 0, 4000)[0] == zz.E_DATA
    assert packets(H, s, 0, 1000, idx, 4000)[0] == zz.E_DATA
