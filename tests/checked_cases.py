"""What the checked range reads' tests share (test_checked_cases_cpu.py on the host, test_gpu_decode_checked.py on the device):
packet-mode streams with their index, sidecar and decoded length, and a list of damaged variants with the verdict a checked read
must give. The yardstick is Python's zlib throughout: the sidecars come from zzflate_amd.packet_checksums_host (zlib.adler32 /
zlib.crc32), and a damage case counts only if zlib itself shows that the damaged packet's checksum differs."""
import ctypes
import os
import random
import zlib
from collections import namedtuple

from conftest import CORPUS
from range_streams import HAND_P, hand_stream

import zzflate_amd as zz

# s: the stream; idx: its packet index; data: its decoded bytes; cks: its sidecar (a list); P, fmt, lvl as written
Stream = namedtuple("Stream", "name fmt lvl P s idx data cks")
# A damaged variant of `stream`: s / cks / total_len as the reader is given them. verdict: "packet" -- E_DATA for a read that touches
# a packet of `bad` (the packets whose decoded bytes differ), the right bytes for a read that does not; "call" -- E_DATA for every
# read, nothing written; "arg" -- E_ARG before any launch.
Damage = namedtuple("Damage", "name stream s cks total_len verdict bad")

HLEN = {0: 2, 1: 10, 2: 0}
TLEN = {0: 4, 1: 8, 2: 0}
CORPUS_BYTES = 100001


def corpus_file(name):
    return open(os.path.join(CORPUS, name), "rb").read()


def oracle_packets(o, data, fmt, lvl, P):
    """the oracle's packet-mode stream and its index (from the sizes of its packets)"""
    s = o.encode_packets(data, fmt, lvl, P, 0)
    npk = max(1, (len(data) + P - 1) // P)
    idx, at = [0], 0
    for k in range(npk):
        ln = max(0, min(P, len(data) - k * P))
        cap = 2 * ln + 1024
        b = ctypes.create_string_buffer(cap)
        at += o.L.zzo_packet_warm(lvl, data, k * P, ln, int(k == npk - 1), b, cap, 0)
        idx.append(at)
    assert len(s) == HLEN[fmt] + at + TLEN[fmt]
    return s, idx


def make(name, fmt, lvl, P, s, idx, data):
    return Stream(name, fmt, lvl, P, s, idx, data, zz.packet_checksums_host(data, fmt, P))


_streams = {}


def streams(o):
    """every intact stream of the list (built once per process)"""
    if "all" in _streams:
        return _streams["all"]
    out = []
    for kind in ("a", "b"):
        s, idx, d = hand_stream(kind)
        out.append(make("hand_" + kind, 0, 1, HAND_P, s, idx, d))
    for name in ("alice29.txt", "kennedy.xls"):
        data = corpus_file(name)[:CORPUS_BYTES]
        for lvl in (0, 1, 2, 3):
            for P, fmt in ((32768, 0), (4096, 1), (1000, 2)):
                s, idx = oracle_packets(o, data, fmt, lvl, P)
                out.append(make(f"{name}_l{lvl}_P{P}", fmt, lvl, P, s, idx, data))
    text = corpus_file("alice29.txt")
    for fmt in (0, 1):
        for label, n in (("empty", 0), ("one_full_packet", 1000), ("P_plus_1", 1001)):
            if n:
                s, idx = oracle_packets(o, text[:n], fmt, 1, 1000)
            else:                                       # one final stored block of no bytes: the empty stream's one empty packet
                empty = b"\x01\x00\x00\xff\xff"
                s = (b"\x78\x01" + empty + b"\x00\x00\x00\x01") if fmt == 0 else (b"\x1f\x8b\x08" + bytes(7) + empty + bytes(8))
                idx = [0, len(empty)]
            out.append(make(f"{label}_f{fmt}", fmt, 1, 1000, s, idx, text[:n]))
    _streams["all"] = out
    return out


def stream(o, name):
    return next(t for t in streams(o) if t.name == name)


def body(t, s=None):
    s = t.s if s is None else s
    return s[HLEN[t.fmt]: len(s) - TLEN[t.fmt]]


def zlib_bytes(t, s):
    """what zlib decodes from the DEFLATE bytes of `s` (the trailer is not looked at), or None"""
    try:
        d = zlib.decompressobj(-15)
        out = d.decompress(body(t, s))
        return out if d.eof and not d.unused_data else None
    except zlib.error:
        return None


def differing_packets(t, got):
    return sorted({k for k in range(len(t.cks)) if got[k * t.P: (k + 1) * t.P] != t.data[k * t.P: (k + 1) * t.P]})


def flip_case(t, at, bit, name):
    """the stream with one bit of its DEFLATE bytes flipped: (Damage or None, decisive). None: zlib refuses the stream or decodes
    another length (such a flip is no candidate); decisive False: it decodes, but no packet's checksum differs."""
    b = bytearray(t.s)
    b[HLEN[t.fmt] + at] ^= bit
    got = zlib_bytes(t, bytes(b))
    if got is None or len(got) != len(t.data):
        return None, True
    cks = zz.packet_checksums_host(got, t.fmt, t.P)
    bad = [k for k in range(len(cks)) if cks[k] != t.cks[k]]
    if not bad or bad != differing_packets(t, got):
        return None, False
    return Damage(name, t, bytes(b), t.cks, len(t.data), "packet", bad), True


_damage = {}


def damages(o):
    """(the damage list, flips generated that decode to the same length, flips among them dropped as indecisive)"""
    if "all" in _damage:
        return _damage["all"]
    out, made, dropped = [], 0, 0
    # a payload byte of a level-0 packet: stored bytes, so exactly that byte changes
    for name in ("alice29.txt_l0_P4096", "kennedy.xls_l0_P32768", "alice29.txt_l0_P1000"):
        t = stream(o, name)
        for k in sorted({0, len(t.cks) // 2, len(t.cks) - 1}):
            c, decisive = flip_case(t, t.idx[k] + 5 + min(17, len(t.data) - k * t.P - 1), 0x20, f"{name}_stored_byte_pk{k}")
            assert c is not None and decisive and c.bad == [k], (name, k)       # a single changed byte changes Adler-32 and CRC-32
            made += 1
            out.append(c)
    # bytes of level-1 and level-2 packets that zlib still decodes to the same length
    for name in ("alice29.txt_l1_P4096", "alice29.txt_l2_P32768", "kennedy.xls_l2_P4096", "alice29.txt_l1_P1000"):
        t = stream(o, name)
        rng = random.Random(sum(name.encode()))
        kept = 0
        for _ in range(4000):
            if kept == 4:
                break
            at = rng.randrange(t.idx[-1])
            c, decisive = flip_case(t, at, 1 << rng.randrange(8), f"{name}_flip_at{at}")
            if c is None and decisive:
                continue
            made += 1
            if c is None:
                dropped += 1
                continue
            kept += 1
            out.append(c)
        assert kept == 4, name
    for name in ("alice29.txt_l1_P32768", "alice29.txt_l2_P4096", "hand_a", "P_plus_1_f1"):
        t = stream(o, name)
        L, npk = len(t.data), len(t.cks)
        # a changed sidecar entry: it no longer folds to the trailer
        for k in sorted({0, npk - 1}):
            cks = list(t.cks); cks[k] ^= 0x100
            out.append(Damage(f"{name}_entry{k}_changed", t, t.s, cks, L, "call", []))
        # a wrong total length: with the right packet count the fold (and gzip's ISIZE) fails, with a wrong one the arguments do
        out.append(Damage(f"{name}_total_len_minus_1", t, t.s, t.cks, L - 1, "call" if (L - 2) // t.P == (L - 1) // t.P else "arg", []))
        out.append(Damage(f"{name}_total_len_plus_P", t, t.s, t.cks, L + t.P, "arg", []))
    # the stream's payload and its entry changed together: every packet matches its entry, the fold does not match the trailer
    for name in ("alice29.txt_l0_P4096", "kennedy.xls_l0_P32768"):
        t = stream(o, name)
        c, _ = flip_case(t, t.idx[1] + 5 + 40, 0x01, "x")
        got = zlib_bytes(t, c.s)
        out.append(Damage(f"{name}_payload_and_entry_changed", t, c.s, zz.packet_checksums_host(got, t.fmt, t.P), len(t.data), "call", [1]))
    # gzip's ISIZE
    t = stream(o, "alice29.txt_l2_P4096")
    b = bytearray(t.s); b[-4] ^= 1
    out.append(Damage("gzip_isize_changed", t, bytes(b), t.cks, len(t.data), "call", []))
    _damage["all"] = (out, made, dropped)
    return _damage["all"]


def touching_range(c):
    """the first damaged packet whole (packet 0 if none is), and a short range in a packet that is intact (None if there is none)"""
    P, L = c.stream.P, len(c.stream.data)
    k = c.bad[0] if c.bad else 0
    hit = (k * P, min(P, L - k * P))
    clean = next((j for j in range(len(c.stream.cks) - 1, -1, -1) if j not in c.bad and j * P < L), None)
    return hit, (None if clean is None else (clean * P + 1, 50))
