"""The single-stream encode forms at the edges of their destination (include/zzflate_amd.h, zz_encode_device): a stream of exactly
`cap` bytes fits and is the roomy call's, one byte less is E_NOSPACE with *out_len all ones -- also where only the trailer does
not fit, and where the header alone fills the room --, nothing outside d_dst[0, cap) is written whatever the result, the next
call on the context is right again, and a refused call leaves no "last call" to verify or index.

The destination is a slice of a larger tensor filled with 0xA5, GUARD bytes of it on either side, at an address that is 1 mod 16
and, in a second pass, 0 mod 16 (the cooperative copy's head and tail): an overrun shows as a changed guard byte, never as a
fault. The sequential level-1 stream, whose block lengths follow from the room, is swept byte by byte around its roomy length
(tests/expansion_cases.py seq_window; tests/test_expansion_cases_cpu.py holds the sweep to its verdict flips): where the
oracle's stream for that capacity inflates, the device writes exactly it, elsewhere it answers E_NOSPACE.
Needs a real MI355X: run with `-m gpu`."""
import ctypes

import numpy as np
import pytest

import expansion_cases as ec
import zzflate_amd as zz

pytestmark = pytest.mark.gpu
GUARD = 4096
P = 4096
SIZES = [1, 65, 4097, 2 * 4096 + 1]
ERR = (1 << 64) - 1
u64, u32 = ctypes.c_uint64, ctypes.c_uint32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctxs(torch):
    return [zz.Context(0), zz.Context(0)]


@pytest.fixture(scope="module")
def inputs(oracle, corpus):
    """[(name, bytes)]: `high`, `uniform` and a corpus prefix at every size, and one input at the stored-fallback threshold"""
    out = [(f"{name}-{n}", d[:n]) for n in SIZES
           for name, d in (("high", ec.high(n, 5)), ("uniform", ec.uniform(n, 5)), ("alice", corpus["alice29.txt"]))]
    k, d = ec.tipping(oracle, 4096, 2, False)[1]              # the last k whose block is stored
    return out + [(f"tipping-k{k}", ec.tip_stream(d, False)[0])]


class Arena:
    """a destination with guards on both sides, inside one allocation"""

    def __init__(self, torch, room, host=False):
        self.torch, self.room, self.host = torch, room, host
        size = GUARD + 16 + room + GUARD
        self.t = np.empty(size, dtype=np.uint8) if host else torch.empty(size, dtype=torch.uint8, device="cuda")
        base = self.t.ctypes.data if host else self.t.data_ptr()
        self.at = {a: GUARD + (a - base - GUARD) % 16 for a in (0, 1)}       # offsets whose address is a mod 16

    def dest(self, align, cap):
        """fill everything, hand out `cap` bytes at an address that is `align` mod 16"""
        assert cap <= self.room
        self.start, self.cap = self.at[align], cap
        if self.host:
            self.t[:] = 0xA5
        else:
            self.t.fill_(0xA5)
            self.torch.cuda.synchronize()
        p = (self.t.ctypes.data if self.host else self.t.data_ptr()) + self.start
        assert p % 16 == align
        return p

    def intact(self):
        """the bytes in front of the destination and from `cap` onward are what they were"""
        if not self.host:
            self.torch.cuda.synchronize()
        a, b = self.t[:self.start], self.t[self.start + self.cap:]
        return bool((a == 0xA5).all()) and bool((b == 0xA5).all())

    def bytes(self, w):
        s = self.t[self.start:self.start + w]
        return s.tobytes() if self.host else s.cpu().numpy().tobytes()


# ---- the forms: f(ctxs, src pointer, n, dst pointer, cap, container) -> (rc, out_len) ---------------------------------------

def _st(c):
    return c._stream()


def f_encode(lvl):
    def f(cs, s, n, d, cap, fmt):
        out = u64(0)
        return zz.lib.zz_encode_device(cs[0]._h, s, n, d, cap, ctypes.byref(out), fmt, lvl, P, _st(cs[0])), out.value
    return f


def f_async(lvl):
    def f(cs, s, n, d, cap, fmt):
        out = u64(0)
        rc = zz.lib.zz_encode_device_async(cs[0]._h, s, n, d, cap, fmt, lvl, P, _st(cs[0]))
        return (rc, ERR) if rc else (zz.lib.zz_encode_finish(cs[0]._h, ctypes.byref(out)), out.value)
    return f


def f_shard(lvl, last):
    def f(cs, s, n, d, cap, fmt):
        out, cks = u64(0), u32(0)
        return zz.lib.zz_encode_shard_device(cs[0]._h, s, n, 0, int(last), d, cap, ctypes.byref(out), ctypes.byref(cks), fmt, lvl, P, _st(cs[0])), out.value
    return f


def f_shard_async(lvl):
    def f(cs, s, n, d, cap, fmt):
        out, cks = u64(0), u32(0)
        rc = zz.lib.zz_encode_shard_device_async(cs[0]._h, s, n, 0, 1, d, cap, fmt, lvl, P, _st(cs[0]))
        return (rc, ERR) if rc else (zz.lib.zz_encode_shard_finish(cs[0]._h, ctypes.byref(out), ctypes.byref(cks), fmt), out.value)
    return f


def f_rerun(lvl):
    """every call reports a violated LDS order and runs again with the call's `cap` (zz_api.hip encode_finish)"""
    inner = f_encode(lvl)

    def f(cs, s, n, d, cap, fmt):
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1
        zz.lib.zz_debug_force_lds_violation(1)
        try:
            return inner(cs, s, n, d, cap, fmt)
        finally:
            zz.lib.zz_debug_force_lds_violation(0)
    return f


def f_ranges(lvl, count):
    def f(cs, s, n, d, cap, fmt):
        out = u64(0)
        return zz.lib.zz_encode_ranges_device(cs[0]._h, s, n, d, cap, ctypes.byref(out), fmt, lvl, count, _st(cs[0])), out.value
    return f


def f_stream(lvl):
    def f(cs, s, n, d, cap, fmt):
        out = u64(0)
        return zz.lib.zz_encode_stream_device(cs[0]._h, s, n, d, cap, ctypes.byref(out), fmt, lvl, _st(cs[0])), out.value
    return f


def f_chunks(lvl):
    def f(cs, s, n, d, cap, fmt):
        out, nch = u64(0), u32(0)
        sizes = (u64 * 64)()
        return zz.lib.zz_encode_stream_chunks_device(cs[0]._h, s, n, d, cap, ctypes.byref(out), fmt, lvl, sizes, 64, ctypes.byref(nch), _st(cs[0])), out.value
    return f


def f_multi(lvl):
    """two shards on two contexts of device 0 where the input has more than one packet, else one"""
    def f(cs, s, n, d, cap, fmt):
        first = ((n - 1) // P + 1) // 2 * P if n > P else 0
        ns = [first, n - first] if first else [n]
        k = len(ns)
        vp = ctypes.c_void_p
        out = u64(0)
        rc = zz.lib.zz_encode_multi_device((vp * k)(*[c._h for c in cs[:k]]), k, (vp * k)(*([s, s + first][:k])), (u64 * k)(*ns), None,
                                           d, cap, ctypes.byref(out), fmt, lvl, P)
        return rc, out.value
    return f


# name -> (form, oracle level, warm window, container pieces?, keeps a last call?, setup); setup: "one-parser", "warm", "extended"
FORMS = {
    "encode-l0": (f_encode(0), 0, 0, True, True, None), "encode-l1": (f_encode(1), 1, 0, True, True, None),
    "encode-l2": (f_encode(2), 2, 0, True, True, None), "encode-l3": (f_encode(3), 3, 0, True, True, None),
    "async-l1": (f_async(1), 1, 0, True, True, None), "async-l2": (f_async(2), 2, 0, True, True, None),
    "shard-l1": (f_shard(1, True), 1, 0, False, True, None), "shard-not-last-l2": (f_shard(2, False), 2, 0, False, True, None),
    "shard-async-l0": (f_shard_async(0), 0, 0, False, True, None), "shard-async-l2": (f_shard_async(2), 2, 0, False, True, None),
    "rerun-l1": (f_rerun(1), 1, 0, True, True, None), "rerun-l2": (f_rerun(2), 2, 0, True, True, None),
    "one-parser-l1": (f_encode(1), 1, 0, True, True, "one-parser"), "one-parser-l2": (f_encode(2), 2, 0, True, True, "one-parser"),
    "warm-l1": (f_encode(1), 1, 4096, True, True, "warm"), "warm-l2": (f_encode(2), 2, 4096, True, True, "warm"),
    "level6": (f_encode(6), 6, 0, True, True, "extended"),
    "ranges-l0": (f_ranges(0, 2), None, 0, True, False, None), "ranges-l2": (f_ranges(2, 2), None, 0, True, False, None),
    "ranges-l3": (f_ranges(3, 3), None, 0, True, False, None),
    "stream-l0": (f_stream(0), None, 0, True, False, None), "stream-l2": (f_stream(2), None, 0, True, False, None),
    "stream-l3": (f_stream(3), None, 0, True, False, None),
    "chunks-l0": (f_chunks(0), None, 0, True, False, None), "chunks-l2": (f_chunks(2), None, 0, True, False, None),
    "chunks-l3": (f_chunks(3), None, 0, True, False, None),
    "multi-l1": (f_multi(1), 1, 0, True, None, None), "multi-l2": (f_multi(2), 2, 0, True, None, None),
}
WHOLE = {"ranges-l0": (0, 2), "ranges-l2": (2, 2), "ranges-l3": (3, 3), "stream-l0": 0, "stream-l2": 2, "stream-l3": 3,
         "chunks-l0": 0, "chunks-l2": 2, "chunks-l3": 3}


def expected(oracle, name, d, fmt):
    """the roomy stream by the oracle"""
    _, lvl, warm, container, _, _ = FORMS[name]
    if name in WHOLE:
        w = WHOLE[name]
        if isinstance(w, tuple):
            return oracle.encode_ranges(d, fmt, *w) if len(d) >= 100 * w[1] else oracle.encode(d, fmt, w[0])
        return oracle.encode_callback(d, fmt, w)[0] if name.startswith("chunks") else oracle.encode(d, fmt, w)
    if container:
        return oracle.encode_packets(d, fmt, lvl, P, warm)
    last = name != "shard-not-last-l2"
    return b"".join(ec.oracle_packet(oracle, d, lvl, off, ln, final and last, warm) for off, ln, final in ec.packets(len(d), P))


def no_last_call(c):
    """zz_verify_last_device and zz_packet_index_device refuse"""
    a, b = u64(0), u64(0)
    return (zz.lib.zz_verify_last_device(c._h, ctypes.byref(a), ctypes.byref(b), _st(c)) == zz.E_ARG and
            zz.lib.zz_packet_index_device(c._h, None, 0, ctypes.byref(a), _st(c)) == zz.E_ARG)


def edges(torch, cs, oracle, name, inputs, call=None, host=False):
    form, _, _, container, keeps_last, _ = FORMS[name] if call is None else (call, None, 0, True, False, None)
    arena = Arena(torch, 2 * max(len(d) for _, d in inputs) + 1024, host)
    bad = []
    for iname, d in inputs:
        n = len(d)
        src = np.frombuffer(d, dtype=np.uint8).copy() if host else torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
        sp = src.ctypes.data if host else src.data_ptr()
        for fmt in range(3):
            hl, tl = (ec.HEADER[fmt], ec.TRAILER[fmt]) if container else (0, 0)
            want = expected(oracle, name, d, fmt) if call is None else oracle.encode_packets(d, fmt, 1, P)
            for align in (1, 0):
                tag = (iname, fmt, align)

                def run(cap):
                    """(rc, out_len, guards intact)"""
                    rc, out = form(cs, sp, n, arena.dest(align, cap), cap, fmt)
                    return rc, out, arena.intact()
                rc, w, ok = run(arena.room)
                if rc != 0 or not ok or arena.bytes(w) != want:
                    bad.append((tag, "roomy", rc, w, len(want), ok))
                    continue
                rc, out, ok = run(w)
                if rc != 0 or out != w or not ok or arena.bytes(w) != want:
                    bad.append((tag, "cap = w", rc, out, ok))
                if keeps_last and cs[0].verify_last() != (0, None):
                    bad.append((tag, "verify_last at cap = w"))
                caps = {w - 1, w - tl - 1} | ({hl - 1, hl} if hl else set())
                for cap in sorted(c for c in caps if 0 <= c < w):
                    rc, out, ok = run(cap)
                    if rc != zz.E_NOSPACE or out != ERR or not ok:
                        bad.append((tag, "cap", cap, rc, out, ok))
                    if keeps_last and not no_last_call(cs[0]):
                        bad.append((tag, "cap", cap, "a refused call left a last call"))
                rc, out, ok = run(arena.room)                    # and the context is as good as new
                if rc != 0 or out != w or not ok or arena.bytes(w) != want:
                    bad.append((tag, "roomy again", rc, out, ok))
    assert bad == [], (name, len(bad), bad[:8])


@pytest.mark.parametrize("name", list(FORMS))
def test_device_forms(torch, ctxs, oracle, inputs, name):
    setup = FORMS[name][5]
    c = ctxs[0]
    try:
        if setup == "one-parser":
            assert zz.lib.zz_debug_lds_order_verdict(0) == 1
            zz.lib.zz_debug_force_lds_order(0)
        c.set_extended_levels(setup == "extended")
        c.set_warm_window(FORMS[name][2])
        edges(torch, ctxs, oracle, name, inputs)
    finally:
        c.set_warm_window(0)
        c.set_extended_levels(False)
        zz.lib.zz_debug_force_lds_order(-1)
        zz.lib.zz_debug_force_lds_violation(0)
        zz.lib.zz_debug_reset_lds_order(0)
        assert zz.lib.zz_debug_lds_order_verdict(0) == 1


def test_host_entry_point(torch, ctxs, oracle, inputs):
    """zz_encode with threaded != 0 into a host buffer of exactly `cap` bytes: *dest_len carries the capacity in and ~0 out"""
    def call(cs, s, n, d, cap, fmt):
        ln = u64(cap)
        cfg = zz._CConfig(fmt, 1, 1)
        return zz.lib.zz_encode(d, ctypes.byref(ln), s, n, ctypes.byref(cfg)), ln.value
    before = zz.lib.zz_get_packet_size()
    try:
        assert zz.lib.zz_set_packet_size(P) == 0
        edges(torch, ctxs, oracle, "host", inputs, call=call, host=True)
    finally:
        zz.lib.zz_set_packet_size(before)


def test_empty_input_and_no_room_at_all(torch, ctxs):
    """n = 0: the one empty block needs its 2 bytes (5 at level 0) and the container's; cap = 0 is refused, the guards stay"""
    arena = Arena(torch, 64)
    src = torch.zeros(16, dtype=torch.uint8, device="cuda")
    bad = []
    for name in ("encode-l0", "encode-l1", "encode-l2", "async-l1", "stream-l1", "stream-l2", "ranges-l2", "multi-l1"):
        form = f_stream(1) if name == "stream-l1" else FORMS[name][0]
        for fmt in range(3):
            for align in (1, 0):
                rc, w = form(ctxs, src.data_ptr(), 0, arena.dest(align, 64), 64, fmt)
                if rc != 0 or not arena.intact() or not ec.inflates(arena.bytes(w), b"", fmt):
                    bad.append((name, fmt, "roomy", rc, w))
                    continue
                for cap, good in ((w, True), (w - 1, False), (0, False)):
                    rc, out = form(ctxs, src.data_ptr(), 0, arena.dest(align, cap), cap, fmt)
                    if (rc, out) != ((0, w) if good else (zz.E_NOSPACE, ERR)) or not arena.intact():
                        bad.append((name, fmt, align, cap, rc, out))
    assert bad == [], bad[:8]


def sweep(torch, ctxs, oracle, form, host):
    """every capacity of the window, three containers, both alignments of the destination"""
    bad, written = [], 0
    for f, n, d in ec.seq_inputs():
        arena = Arena(torch, 2 * n + 1024, host)
        src = np.frombuffer(d, dtype=np.uint8).copy() if host else torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
        sp = src.ctypes.data if host else src.data_ptr()
        for fmt in range(3):
            for cap in ec.seq_window(oracle, d, fmt):
                want = ec.seq_expected(oracle, d, fmt, cap)
                align = cap & 1
                rc, out = form(ctxs, sp, n, arena.dest(align, cap), cap, fmt)
                if not arena.intact():
                    bad.append((f, n, fmt, cap, "guard"))
                if want is None:
                    if rc != zz.E_NOSPACE or out != ERR:
                        bad.append((f, n, fmt, cap, "accepted", rc, out))
                elif rc != 0 or out != len(want) or arena.bytes(out) != want:
                    bad.append((f, n, fmt, cap, "bytes", rc, out, len(want)))
                else:
                    written += 1
    assert bad == [] and written > 300, (len(bad), bad[:8], written)


def test_sequential_level1_capacity_sweep(torch, ctxs, oracle):
    sweep(torch, ctxs, oracle, f_stream(1), False)


def test_sequential_level1_capacity_sweep_through_the_host_entry_point(torch, ctxs, oracle):
    def call(cs, s, n, d, cap, fmt):
        ln = u64(cap)
        cfg = zz._CConfig(fmt, 1, 0)
        return zz.lib.zz_encode(d, ctypes.byref(ln), s, n, ctypes.byref(cfg)), ln.value
    sweep(torch, ctxs, oracle, call, True)
