"""Files, indexes and reads for the tests of zz_decode_members_ranges_device (tests/test_members_ranges_cases_cpu.py on the host
rules, tests/test_gpu_decode_members_ranges.py on the device), built with members_cases' builders and zlib, and the yardstick
every read is held to: zlib's verdict on each member the index cuts out, member by member."""
import functools
import random
import zlib

import members_cases as mc

STAGE = 64 << 20                    # ZZ_MR_STAGE
OK, E_NOSPACE, E_ARG, E_UNSUPPORTED, E_DATA = 0, -2, -4, -5, -6
GUARD = 32
U64 = 1 << 64


def build(members, tail=b""):
    """(file, index) of a list of (member bytes, decoded length): the index from the members' lengths; `tail` follows the file
    behind the index's last offset"""
    idx, c, u = [], 0, 0
    for m, n in members:
        idx.append((c, u))
        c += len(m)
        u += n
    idx.append((c, u))
    return b"".join(m for m, _ in members) + tail, idx


def mem(data, level=6):
    return mc.bgzf(data, level), len(data)


EMPTY = (mc.EOF_BLOCK, 0)


@functools.lru_cache(maxsize=None)
def good_files():
    """(name, file, index): every member is what the index says"""
    rng = random.Random(15)
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), mc.corpus("fields.c")[:5000]
    stored = bytes(rng.getrandbits(8) for _ in range(65280))
    out = []
    out.append(("uneven members",) + build([mem(b"x"), mem(b"yz"), mem(stored, 0), mem(mc.text(65536, 3)), EMPTY]))
    out.append(("empty members first, in the middle, twice in a row and last",) + build([EMPTY, mem(a), EMPTY, EMPTY, mem(b), mem(c), EMPTY]))
    out.append(("one member alone",) + build([mem(a)]))
    out.append(("300 members of 100 bytes",) + build([mem(mc.text(100, k)) for k in range(300)] + [EMPTY]))
    out.append(("no EOF block",) + build([mem(a), mem(b, 1), mem(c)]))
    out.append(("a piece: the index ends in front of src_len",) + build([mem(a), mem(b)], tail=mc.bgzf(c) + mc.EOF_BLOCK))
    return out


def three():
    a, b, c = mc.text(3000, 1), mc.text(9000, 2), mc.corpus("fields.c")[:5000]
    return a, b, c


@functools.lru_cache(maxsize=None)
def damaged_files():
    """(name, file, index): one member is not what the index says; the others are"""
    a, b, c = three()
    out = []
    m = bytearray(mc.bgzf(b, 0))
    m[18 + 5 + 100] ^= 0x40                                   # a data byte of the stored block: the structure stands, the CRC fails
    out.append(("a stored member with one data byte changed",) + build([mem(a), (bytes(m), len(b)), mem(c), EMPTY]))
    m = bytearray(mc.bgzf(b))
    m[-4] ^= 1
    out.append(("a member with a wrong ISIZE",) + build([mem(a), (bytes(m), len(b)), mem(c), EMPTY]))
    out.append(("a member truncated with BSIZE adjusted",) + build([mem(a), (mc.bgzf_open(b, 6, 40), len(b)), mem(c), EMPTY]))
    return out


@functools.lru_cache(maxsize=None)
def lying_indexes():
    """(name, file, index): a good file under an index that lies at one place"""
    a, b, c = three()
    file, idx = build([mem(a), mem(b, 1), mem(c), EMPTY])
    out = []

    def lie(name, j, dc, du):
        bad = list(idx)
        bad[j] = (bad[j][0] + dc, bad[j][1] + du)
        out.append((name, file, bad))
    lie("a decoded offset one too large", 1, 0, 1)
    lie("a decoded offset one too small", 2, 0, -1)
    lie("a file offset one too large", 1, 1, 0)
    lie("a file offset one too small", 2, -1, 0)
    lie("u descending at one entry", 2, 0, -(len(b) + 1))
    lie("u_0 = 1", 0, 0, 1)
    lie("a last file offset of src_len + 1", len(idx) - 1, 1, 0)
    lie("c not strictly ascending", 2, -len(mc.bgzf(b, 1)), 0)
    big = [(cj, uj + (STAGE + 1 if j >= 3 else 0)) for j, (cj, uj) in enumerate(idx)]       # member 2's room passes the stage
    out.append(("a room above the stage", file, big))
    return out


def index_ok(file, idx):
    c, u = [p[0] for p in idx], [p[1] for p in idx]
    return (u[0] == 0 and all(x < y for x, y in zip(c, c[1:])) and all(x <= y for x, y in zip(u, u[1:])) and c[-1] <= len(file))


def reads_for(idx):
    """(first, nbytes, cap) for an index; cap None: exactly m"""
    u = [p[1] for p in idx]
    L = u[-1]
    rooms = [y - x for x, y in zip(u, u[1:])]
    reads = []
    for e in sorted(set(u)):
        for d in (-1, 0, 1):
            for n in (0, 1, 2):
                if e + d >= 0:
                    reads.append((e + d, n, None))
    ne = [j for j, r in enumerate(rooms) if 0 < r <= STAGE]
    if len(ne) >= 3:
        reads.append((u[ne[1]] - 1, rooms[ne[1]] + 2, None))          # crosses three members
    reads += [(0, L, None), (L, 10, None), (L + 1, 1, None), (min(1, L), U64 - 1, None), (U64 - 1, 2, None), (L // 2, 1 << 40, None)]
    for first, n in ((L // 3, 1000), (0, 1)):
        m = max(0, min(n, L - first))
        reads += [(first, n, m), (first, n, m - 1), (first, n, 0)] if m else [(first, n, 0)]
    j = max(ne, key=lambda k: rooms[k]) if ne else 0
    if ne:
        for i in range(64):                                           # 64 reads inside one member
            reads.append((u[j] + (i * 37) % rooms[j], 1 + i % 3, None))
    reads += [(10, 50, None), (30, 50, None), (0, 60, None)]          # reads that overlap each other
    return reads


def plan(idx, first, nbytes, cap):
    """(status, m, cap) by the plan's rules; cap None becomes m"""
    L = idx[-1][1]
    if first > L or first + nbytes >= U64:
        return E_ARG, 0, 0 if cap is None else cap
    m = min(nbytes, L - first)
    cap = m if cap is None else max(cap, 0)
    return (E_NOSPACE if m > cap else OK), m, cap


class Judge:
    """zlib's verdict on the members an index cuts out of a file, each asked once"""

    def __init__(self, file, idx, stage=STAGE):
        self.file, self.idx, self.stage, self.seen = file, idx, stage, {}
        self.valid = index_ok(file, idx)

    def member(self, j):
        """the member's bytes if it is what the index says, else None"""
        if j not in self.seen:
            (c0, u0), (c1, u1) = self.idx[j], self.idx[j + 1]
            out = None
            try:
                d = zlib.decompressobj(31)
                got = d.decompress(self.file[c0:c1])
                if d.eof and not d.unused_data and len(got) == u1 - u0:
                    out = got
            except zlib.error:
                pass
            self.seen[j] = out
        return self.seen[j]

    def read(self, first, nbytes, cap):
        """(status, bytes or None)"""
        if not self.valid:
            return E_DATA, None
        st, m, cap = plan(self.idx, first, nbytes, cap)
        if st != OK:
            return st, None
        if m == 0:
            return OK, b""
        u = [p[1] for p in self.idx]
        touched = [j for j in range(len(u) - 1) if u[j + 1] > u[j] and u[j] < first + m and u[j + 1] > first]
        small = [j for j in touched if u[j + 1] - u[j] <= self.stage]
        if any(self.member(j) is None for j in small):
            return E_DATA, None
        if len(small) != len(touched):
            return E_UNSUPPORTED, None
        whole = b"".join(self.member(j) for j in touched)
        at = first - u[touched[0]]
        return OK, whole[at:at + m]

    def call(self, reads):
        """(return code, [(status, bytes)])"""
        res = [self.read(*r) for r in reads]
        sts = {s for s, _ in res}
        rc = next((e for e in (E_DATA, E_UNSUPPORTED, E_ARG, E_NOSPACE) if e in sts), OK)
        return rc, res

    def decoded(self, reads):
        """members a call decodes: the touched ones below the stage's limit, each once"""
        if not self.valid:
            return 0
        u = [p[1] for p in self.idx]
        seen = set()
        for first, nbytes, cap in reads:
            st, m, _ = plan(self.idx, first, nbytes, cap)
            if st == OK and m:
                seen |= {j for j in range(len(u) - 1) if 0 < u[j + 1] - u[j] <= self.stage and u[j] < first + m and u[j + 1] > first}
        return len(seen)


def all_cases():
    """(name, file, index, reads) of every good, damaged and lying-index case"""
    out = []
    for name, file, idx in good_files() + damaged_files() + lying_indexes():
        if idx[-1][1] > STAGE:                                 # (reads and caps by the file's honest length: a lying L would ask for 64 MiB each)
            honest = [(c, u - (STAGE + 1 if j >= 3 else 0)) for j, (c, u) in enumerate(idx)]
            out.append((name, file, idx, [(f, n, plan(honest, f, n, cap)[2]) for f, n, cap in reads_for(honest)]))
        else:
            out.append((name, file, idx, reads_for(idx)))
    return out


def layout(reads, idx):
    """where read r's destination lies in one buffer: GUARD bytes, cap bytes, GUARD bytes, and the destination's address has
    residue r mod 16 when the buffer's has residue 0. Returns (offsets of the destinations, caps, buffer size)."""
    offs, caps, at = [], [], 0
    for r, (first, nbytes, cap) in enumerate(reads):
        _, _, cp = plan(idx, first, nbytes, cap)
        at += GUARD
        at += (r % 16 - at) % 16
        offs.append(at)
        caps.append(cp)
        at += cp + GUARD
    return offs, caps, at + 16
