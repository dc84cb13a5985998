"""Member files for the tests of zz_decode_members_device (tests/test_inflate_members_cpu.py on the host rules,
tests/test_gpu_decode_members.py on the device): gzip members built in Python -- raw deflate by zlib, hand-made headers -- and
the yardstick every verdict is held to: zlib's own loop over the members."""
import gzip
import os
import random
import struct
import zlib

CORPUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpus")
BLOCKED, WALKED, SERIAL = 1, 2, 3
STRETCH = 4096                      # ZZ_MEM_STRETCH: source bytes per workgroup of the mark pass
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")     # bgzip's empty last member


def corpus(name):
    with open(os.path.join(CORPUS, name), "rb") as f:
        return f.read()


def yardstick(file):
    """The decoded bytes as zlib reads the file member by member, or None where it refuses (an empty file, any zlib error, a
    member that does not end)."""
    if not file:
        return None
    out, rest = [], file
    try:
        while rest:
            d = zlib.decompressobj(31)
            out.append(d.decompress(rest))
            if not d.eof:
                return None
            rest = d.unused_data
    except zlib.error:
        return None
    return b"".join(out)


def checked(file):
    """yardstick(file), after holding it to gzip.decompress on what it accepts"""
    want = yardstick(file)
    if want is not None:
        assert gzip.decompress(file) == want, "the yardstick and gzip.decompress disagree"
    return want


def raw_deflate(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def member(data, level=6, extra=None, name=None, comment=None, hcrc=False):
    """a gzip member with a hand-made header; `extra` is the whole extra field"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + raw_deflate(data, level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def bgzf(data, level=6, before=b"", after=b"", bsize_error=0, **fields):
    """a blocked member: the `BC` subfield announces the member's length - 1 (+ bsize_error); `before` / `after` are other
    subfields around it"""
    placeholder = member(data, level, extra=before + b"BC\x02\x00\x00\x00" + after, **fields)
    bsize = len(placeholder) - 1 + bsize_error
    assert 0 <= bsize < 65536, "the member does not fit BSIZE"
    m = member(data, level, extra=before + b"BC\x02\x00" + struct.pack("<H", bsize) + after, **fields)
    assert len(m) == len(placeholder)
    return m


def bgzf_open(data, level, keep):
    """a damaged blocked member: nothing but the first `keep` bytes of its blocks behind the header, BSIZE announcing the length
    it has now -- a decoder is still inside a block when the member's bytes end, and goes on into whatever follows it"""
    m = bytearray(bgzf(data, level)[:18 + keep])
    m[16:18] = struct.pack("<H", len(m) - 1)
    return bytes(m)


def produced(rest):
    """bytes zlib gets out of the (damaged) member at the head of `rest` before it must refuse it: the largest k for which it
    hands out k bytes without an error. With less room than that the member's bytes pass the room first (no space); with that
    much or more it is found invalid (data)."""
    k = 0
    while True:
        try:
            if len(zlib.decompressobj(31).decompress(rest, k + 1)) < k + 1:
                return k
        except zlib.error:
            return k
        k += 1


def open_member_files(step):
    """(file, bytes in front of the damaged member, bytes it produces): a good member, a member cut inside a block at every
    `step`-th place, and a follower whose bytes the decoder runs into"""
    a, b, c = text(100, 1), text(500, 2), text(200, 3)
    for level in (6, 1):
        whole = len(bgzf(b, level)) - 18 - 8
        for keep in range(12, whole, step):
            for follower in (bgzf(c), b"\x00" * 40, b"\xff" * 40, b"\xaa" * 40, b"\x1f\x8b" * 20):
                bad = bgzf_open(b, level, keep)
                yield bgzf(a) + bad + follower, len(a), produced(bad + follower)


def subfield(si, payload):
    return si + struct.pack("<H", len(payload)) + payload


def bgzf_sized(size, rng):
    """a blocked member of exactly `size` bytes (at least BGZF_MIN): stored random bytes and a filler subfield in front of `BC`"""
    data = bytes(rng.getrandbits(8) for _ in range(8))
    base = len(bgzf(data, 0, before=subfield(b"ZZ", b"")))
    assert size >= base
    m = bgzf(data, 0, before=subfield(b"ZZ", b"\x00" * (size - base)))
    assert len(m) == size
    return m


BGZF_MIN = 18 + 4 + 5 + 8 + 8         # header with BC, an empty filler subfield, one stored block of eight bytes, trailer


def text(n, seed=0):
    t = corpus("alice29.txt")
    start = (seed * 7919) % (len(t) - n) if n < len(t) else 0
    return (t * (n // len(t) + 1))[start:start + n]


def path_cases():
    """(name, file, path the device must report) -- every file here is valid"""
    rng = random.Random(5)
    a, b, c = text(3000, 1), text(9000, 2), corpus("fields.c")[:5000]
    cases = []
    cases.append(("one member", bgzf(a), BLOCKED))
    big = bytes(rng.getrandbits(8) for _ in range(65280))           # stored at level 0: 65,280 input bytes fit one member
    cases.append(("members of 1, 4096 and 65280 input bytes", bgzf(b"x") + bgzf(text(4096, 3)) + bgzf(big, 0), BLOCKED))
    cases.append(("empty member at the end", bgzf(a) + bgzf(b) + EOF_BLOCK, BLOCKED))
    cases.append(("empty member in the middle", bgzf(a) + EOF_BLOCK + bgzf(b) + EOF_BLOCK, BLOCKED))
    cases.append(("BC behind two other subfields",
                  bgzf(a, before=subfield(b"AB", b"hello") + subfield(b"XY", b"")) + bgzf(b, before=subfield(b"BC", b"abc") + subfield(b"Q\x00", b"\x01\x02"), after=subfield(b"BC", b"\x00\x00")),
                  BLOCKED))
    for lvl in (0, 1, 6, 9):
        cases.append((f"level {lvl}", bgzf(a, lvl) + bgzf(b, lvl) + bgzf(c, lvl) + EOF_BLOCK, BLOCKED))
    # a member that stores, at level 0, a complete small blocked file: its headers are candidates, not members
    small = bgzf(text(500, 4)) + bgzf(text(700, 5)) + EOF_BLOCK
    cases.append(("a stored blocked file in the middle", bgzf(a) + bgzf(small, 0) + bgzf(b) + EOF_BLOCK, WALKED))
    cases.append(("a stored blocked file in the first member", bgzf(small, 0) + bgzf(a) + bgzf(b), WALKED))
    cases.append(("a stored blocked file in the last member", bgzf(a) + bgzf(b) + bgzf(small, 0), WALKED))
    cases.append(("python gzip members without an extra field", gzip.compress(a) + gzip.compress(b), SERIAL))
    cases.append(("the middle member lacks BC", bgzf(a) + member(b) + bgzf(c), SERIAL))
    cases.append(("FNAME, FCOMMENT and FHCRC members", member(a, name=b"a.txt") + member(b, comment=b"the second") + member(c, hcrc=True)
                  + member(a, extra=b"", name=b"n", comment=b"c", hcrc=True), SERIAL))
    cases.append(("blocked members with FNAME and FHCRC", bgzf(a, name=b"a.txt", hcrc=True) + bgzf(b, comment=b"c") + EOF_BLOCK, BLOCKED))
    cases.append(("BSIZE one too small", bgzf(a) + bgzf(b, bsize_error=-1) + bgzf(c), SERIAL))
    cases.append(("BSIZE one too large", bgzf(a) + bgzf(b, bsize_error=1) + bgzf(c), SERIAL))
    cases.append(("BSIZE one too large in the last member", bgzf(a) + bgzf(b, bsize_error=1), SERIAL))
    return cases


def three_members():
    """a three-member blocked file of about 200 bytes and its members' lengths"""
    ms = [bgzf(b"first member, "), bgzf(b"the second one is a little longer than the first, "), bgzf(b"and the third.")]
    return b"".join(ms), [len(m) for m in ms]


def refusal_cases():
    """(name, file): zlib refuses every one of them"""
    a, b, c = text(3000, 1), text(9000, 2), corpus("fields.c")[:5000]
    ms = [bgzf(a), bgzf(b), bgzf(c)]
    good = b"".join(ms)
    starts = [0, len(ms[0]), len(ms[0]) + len(ms[1])]
    cases = []

    def flipped(pos, bit=0):
        f = bytearray(good); f[pos] ^= 1 << bit
        return bytes(f)
    for k, nm in enumerate(("member 0", "the middle member", "the last member")):
        end = starts[k] + len(ms[k])
        cases.append((f"a flipped CRC in {nm}", flipped(end - 8)))
    cases.append(("a flipped ISIZE", flipped(starts[1] + len(ms[1]) - 4)))
    cases.append(("a flipped bit inside a member's blocks", flipped(starts[1] + 18 + 200, 3)))
    cases.append(("one zero byte behind the last member", good + b"\x00"))
    cases.append(("eight zero bytes behind the last member", good + b"\x00" * 8))
    cases.append(("one byte between members", ms[0] + b"\x00" + ms[1] + ms[2]))
    cases.append(("an empty file", b""))
    cases.append(("a zlib stream", zlib.compress(a)))
    cases.append(("a plain member with a flipped CRC behind a good one", gzip.compress(a) + gzip.compress(b)[:-8] + b"\x00" * 4 + gzip.compress(b)[-4:]))
    return cases
