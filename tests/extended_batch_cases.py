"""Inputs and expectations for levels 4..6 of zz_encode_batch_flags_device and zz_encode_members_device with their extended
switch (tests/test_extended_batch_cases_cpu.py guards the list without a GPU, tests/test_gpu_encode_extended_batch.py holds the
device to it). The yardstick is the oracle: item i of a batch is oracle.encode_packets(item, format, level, P) of the item
ALONE -- packet k sees min(k * P, 8192) bytes of its own item at level 4 and min(k * P, 32768) at levels 5, 6, and nothing in
front of the item; a member is members_write_cases.expected(...) at the same level."""
import functools
import random
import struct
import zlib

import members_write_cases as mw
from conftest import synth

LEVELS = [4, 5, 6]
PACKETS = [32768, 4096]
ZLIB, GZIP, DEFLATE = 0, 1, 2
FORMATS = [ZLIB, GZIP, DEFLATE]
WBITS = {ZLIB: 15, GZIP: 31, DEFLATE: -15}
COPY = 6000                          # bytes of X in the copy-in-front cases


def lengths(P):
    """what goes wrong where: target = n - 16 is 0, 1 or 4; the first 64-position block edge; the packet edges at 4096 and at
    32768 (a 1-byte last packet); BGZF's two packets; 3P + 5: the level-4 window grows 0, 4096, 8192, 8192 at P = 4096"""
    return [0, 1, 4, 15, 16, 17, 20, 63, 64, 65, 80, 4095, 4096, 4097, 32767, 32768, 32769, 65280, 65537, 3 * P + 5]


@functools.lru_cache(maxsize=None)
def items(P):
    """the whole list of one call: text of every length, one random item (it takes the stored fallback), 70,000 zeros (one hash
    bucket, the longest chains)"""
    out = [mw.text(n, 3 + i) for i, n in enumerate(lengths(P))]
    out.append(synth("random", 20000, 5))
    out.append(bytes(70000))
    return out


def random_items(P):
    """indices into items(P) of the items that are meant to be stored"""
    return [len(lengths(P))]


def empty_stream(fmt):
    """an empty item: the container around the empty final block (fixed) that the batch call writes at level 2"""
    if fmt == ZLIB:
        return b"\x78\x01" + b"\x03\x00" + struct.pack(">I", 1)
    if fmt == GZIP:
        return bytes.fromhex("1f8b08000000000000ff") + b"\x03\x00" + struct.pack("<II", 0, 0)
    return b"\x03\x00"


def expected_item(oracle, d, fmt, level, P):
    return oracle.encode_packets(d, fmt, level, P) if d else empty_stream(fmt)


@functools.lru_cache(maxsize=None)
def expected_items(oracle, fmt, level, P):
    """expected streams of items(P), computed once and shared"""
    return [expected_item(oracle, d, fmt, level, P) for d in items(P)]


def inflate(stream, fmt):
    o = zlib.decompressobj(WBITS[fmt])
    out = o.decompress(stream)
    assert o.eof and not o.unused_data
    return out


def stored_blocks_only(raw):
    """True where a raw-deflate stream holds stored blocks and nothing else (walks the stored block headers)"""
    at = 0
    while True:
        if at + 5 > len(raw) or raw[at] & 6:
            return False
        ln, nl = struct.unpack_from("<HH", raw, at + 1)
        if ln ^ nl != 0xFFFF:
            return False
        final = raw[at] & 1
        at += 5 + ln
        if final:
            return at == len(raw)


@functools.lru_cache(maxsize=None)
def copy_cases():
    """(name, X): one buffer holds X || X || X, its thirds are three items (or three members of block_size = COPY); every one
    must come out as the stream of X alone. A window that leaks across an item's start finds all of X one copy back."""
    return [("text", mw.text(COPY, 9)), ("random", synth("random", COPY, 9))]


@functools.lru_cache(maxsize=None)
def many_items():
    """700 items of 1..6,000 bytes, seeded: slices of one text at any offset"""
    rng = random.Random(700)
    long = mw.text(60000, 2)
    out = []
    for _ in range(700):
        n = rng.randint(1, 6000)
        o = rng.randrange(0, len(long) - n)
        out.append(long[o:o + n])
    return out
