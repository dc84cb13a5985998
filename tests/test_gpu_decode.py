"""Decode on the device (zz_decode_device): round trips through the indexed, discovered and serial paths, streams made
by the oracle, by Python's zlib / gzip and by the library's other encoders, errors, and full-size calls."""
import gzip
import os
import random
import zlib

import pytest

from conftest import CORPUS, SYNTH_KINDS, Oracle, synth

torch = pytest.importorskip("torch")
import zzflate_amd as zz  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = zz.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def xctx():
    c = zz.Context(0)
    c.set_extended_levels(True)
    yield c
    c.close()


def dev(data):
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def encode(c, src, n, fmt, lvl, P):
    cap = zz.bound(n, fmt, min(lvl, 3), P) + 64
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = c.encode(src, n, dst, cap, fmt, lvl, P)
    return dst[:w].clone(), w


def decode(c, stream, w, n, fmt, P, index=None, slack=64):
    cap = n + slack
    out = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    got = c.decode(stream, w, out, cap, fmt, P, index)
    return out, got


def roundtrip(c, data, fmt, lvl, P, path=zz.DECODE_INDEXED):
    n = len(data)
    src = dev(data)
    stream, w = encode(c, src, n, fmt, lvl, P)
    idx = c.packet_index()
    out, got = decode(c, stream, w, n, fmt, P, idx)
    assert got == n
    assert torch.equal(out[:n], src[:n])
    assert c.last_decode_path() == path
    return stream, w, idx


def corpus_file(name):
    return open(os.path.join(CORPUS, name), "rb").read()


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_roundtrip_corpus(ctx, lvl, fmt):
    for name in ("alice29.txt", "kennedy.xls", "ptt5", "fields.c"):
        roundtrip(ctx, corpus_file(name), fmt, lvl, 32768)


@pytest.mark.parametrize("kind", SYNTH_KINDS + ["longperiod"])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_roundtrip_synthetic(ctx, kind, lvl):
    for P in (32768, 4096):
        roundtrip(ctx, synth(kind, 100000, 3), 0, lvl, P)


@pytest.mark.parametrize("P", [32768, 4096, 1000, 1])
@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_roundtrip_sizes(ctx, P, lvl):
    base = synth("words", 3 * max(P, 1000) + 10, 5)
    for n in sorted({0, 1, max(P - 1, 0), P, P + 1}):
        roundtrip(ctx, base[:n], 0 if n % 2 else 1, lvl, P)


@pytest.mark.parametrize("warm", [4096, 32768])
@pytest.mark.parametrize("lvl", [1, 2, 3])
def test_roundtrip_warm(lvl, warm):
    c = zz.Context(0)
    c.set_warm_window(warm)
    data = corpus_file("lcet10.txt") + synth("period", 50000, 7)
    for P in (32768, 4096, 1000):
        roundtrip(c, data, 1, lvl, P)
    c.close()


@pytest.mark.parametrize("lvl", [4, 5, 6])
def test_roundtrip_extended(xctx, lvl):
    data = corpus_file("alice29.txt") + synth("period", 60000, 2) + corpus_file("kennedy.xls")[:100000]
    for P in (32768, 4096, 1000):
        for fmt in (0, 1, 2):
            roundtrip(xctx, data, fmt, lvl, P)


def test_pending_bytes_are_resolved(xctx):
    """Periodic data at level 6 with small packets: almost every packet copies from the one in front of it."""
    data = synth("period", 300000, 11)
    roundtrip(xctx, data, 0, 6, 1000)
    pend, rounds = xctx.last_decode_stats()
    assert pend > 100000 and rounds >= 2


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_discovery_recovers_the_index(ctx, lvl):
    for P in (32768, 4096, 1000):
        data = corpus_file("lcet10.txt")[: 5 * P + 17] if P > 1000 else synth("words", 20000, 1)
        stream, w, idx = roundtrip(ctx, data, 0, lvl, P)
        out, got = decode(ctx, stream, w, len(data), 0, P, None)
        assert got == len(data) and torch.equal(out[: len(data)], dev(data)[: len(data)])
        assert ctx.last_decode_path() == zz.DECODE_DISCOVERED
        assert torch.equal(ctx.last_decode_index(), idx)


def marker_data(n, seed):
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.getrandbits(8) for _ in range(rng.randint(500, 3000))) + b"\x01\x00\xfe\xff" + bytes([rng.getrandbits(8)])
    return bytes(out[:n])


@pytest.mark.parametrize("lvl", [0, 2])
def test_discovery_with_markers_inside_stored_data(ctx, lvl):
    """False candidates (the marker inside stored bytes) are walked over and phase 1 runs again on the recovered index,
    with a destination just the size of the output."""
    data = marker_data(150000, lvl)
    src = dev(data)
    for P in (32768, 4096):
        stream, w = encode(ctx, src, len(data), 0, lvl, P)
        idx = ctx.packet_index()
        assert bytes(stream.cpu().numpy()).count(b"\x01\x00\xfe\xff") > len(data) // P + 10
        for slack in (0, 64):
            out, got = decode(ctx, stream, w, len(data), 0, P, None, slack=slack)
            assert got == len(data) and torch.equal(out[: len(data)], src)
            assert ctx.last_decode_path() == zz.DECODE_DISCOVERED
            assert torch.equal(ctx.last_decode_index(), idx)


def test_nospace_is_found_by_the_parallel_paths(ctx):
    data = corpus_file("lcet10.txt")
    src = dev(data)
    n = len(data)
    stream, w = encode(ctx, src, n, 0, 2, 4096)
    idx = ctx.packet_index()
    for cap in (n - 1, n - 5000, 100):
        for index in (idx, None):
            out = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            expect(zz.E_NOSPACE, lambda: ctx.decode(stream, w, out, cap, 0, 4096, index))
            assert bool((out[cap:] == 0x5A).all())
            assert "destination too small for the decoded stream (%d bytes)" % n in zz.lib.zz_last_error().decode()


def test_index_must_be_an_int64_tensor_on_the_device(ctx):
    data = corpus_file("fields.c")
    src = dev(data)
    stream, w = encode(ctx, src, len(data), 0, 1, 4096)
    idx = ctx.packet_index()
    out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        ctx.decode(stream, w, out, len(data) + 64, 0, 4096, idx.to(torch.int32))
    with pytest.raises(TypeError):
        ctx.decode(stream, w, out, len(data) + 64, 0, 4096, torch.stack([idx, idx], 1)[:, 0])
    with pytest.raises(ValueError):
        ctx.decode(stream, w, out, len(data) + 64, 0, 4096, idx.cpu())
    assert ctx.decode(stream, w, out, len(data) + 64, 0, 4096, idx) == len(data)


def test_candidates_over_the_cap_go_serial(ctx):
    data = b"\x01\x00\xfe\xff" * 20000
    src = dev(data)
    stream, w = encode(ctx, src, len(data), 0, 0, 32768)
    out, got = decode(ctx, stream, w, len(data), 0, 32768, None)
    assert got == len(data) and torch.equal(out[: len(data)], src)
    assert ctx.last_decode_path() == zz.DECODE_SERIAL


def oracle_index(o, data, lvl, P):
    import numpy as np
    offs, at = [0], 0
    npk = max(1, (len(data) + P - 1) // P)
    for k in range(npk):
        ln = min(P, len(data) - k * P)
        at += len(o.packet(data, lvl, k * P, ln, k == npk - 1))
        offs.append(at)
    return torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_oracle_streams_all_paths(ctx, lvl):
    o = Oracle()
    for name, P in (("alice29.txt", 32768), ("kennedy.xls", 4096), ("fields.c", 1000)):
        data = corpus_file(name)
        s = o.encode_packets(data, 0, lvl, P)
        idx = oracle_index(o, data, lvl, P)
        assert int(idx[-1]) == len(s) - 6
        st = dev(s)
        for P2, index, path in ((P, idx, zz.DECODE_INDEXED), (P, None, zz.DECODE_DISCOVERED), (0, None, zz.DECODE_SERIAL)):
            out, got = decode(ctx, st, len(s), len(data), 0, P2, index)
            assert got == len(data) and bytes(out[: len(data)].cpu().numpy()) == data
            assert ctx.last_decode_path() == path


@pytest.mark.parametrize("lvl", [0, 1, 6, 9])
def test_serial_python_zlib_and_gzip(ctx, lvl):
    data = corpus_file("alice29.txt") + corpus_file("ptt5")
    for wbits, fmt in ((15, 0), (31, 1), (-15, 2)):
        co = zlib.compressobj(lvl, zlib.DEFLATED, wbits)
        s = co.compress(data) + co.flush()
        for P in (0, 32768):
            out, got = decode(ctx, dev(s), len(s), len(data), fmt, P)
            assert got == len(data) and bytes(out[: len(data)].cpu().numpy()) == data
            # (with a packet size, discovery may take a stream whose blocks happen to line up with it)
            assert ctx.last_decode_path() == zz.DECODE_SERIAL or P
    s = gzip.compress(data, compresslevel=max(lvl, 1))
    out, got = decode(ctx, dev(s), len(s), len(data), 1, 0)
    assert bytes(out[: len(data)].cpu().numpy()) == data


def test_gzip_header_fields(ctx):
    data = corpus_file("fields.c")
    body = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = body.compress(data) + body.flush()
    hdr = bytearray(b"\x1f\x8b\x08\x1e\x00\x00\x00\x00\x00\xff")   # FEXTRA FNAME FCOMMENT FHCRC
    hdr += b"\x03\x00abc" + b"name.txt\x00" + b"a comment\x00"
    crc = zlib.crc32(bytes(hdr)) & 0xFFFF
    hdr += bytes([crc & 0xFF, crc >> 8])
    s = bytes(hdr) + raw + zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little")
    out, got = decode(ctx, dev(s), len(s), len(data), 1, 0)
    assert got == len(data) and bytes(out[:got].cpu().numpy()) == data


@pytest.mark.parametrize("lvl", [0, 2, 3])
def test_serial_sequential_and_ranges_streams(ctx, lvl):
    data = corpus_file("lcet10.txt")
    src = dev(data)
    cap = 2 * len(data) + 4096
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode_stream(src, len(data), dst, cap, 0, lvl)
    for P in (0, 32768):
        out, got = decode(ctx, dst[:w].clone(), w, len(data), 0, P)
        assert got == len(data) and torch.equal(out[: len(data)], src)
    w = ctx.encode_ranges(src, len(data), dst, cap, 7, 1, lvl)
    out, got = decode(ctx, dst[:w].clone(), w, len(data), 1, 0)
    assert got == len(data) and torch.equal(out[: len(data)], src)
    assert ctx.last_decode_path() == zz.DECODE_SERIAL


def expect(code, fn):
    with pytest.raises(zz.ZzFlateError) as e:
        fn()
    assert e.value.code == code, str(e.value)


def test_errors(ctx):
    data = corpus_file("alice29.txt")
    src = dev(data)
    n = len(data)
    for fmt in (0, 1):
        stream, w = encode(ctx, src, n, fmt, 2, 4096)
        idx = ctx.packet_index()
        raw = bytearray(stream.cpu().numpy().tobytes())
        bad = bytearray(raw); bad[-(4 if fmt == 0 else 8)] ^= 0x40            # the checksum
        expect(zz.E_DATA, lambda: decode(ctx, dev(bytes(bad)), w, n, fmt, 4096, idx))
        expect(zz.E_DATA, lambda: decode(ctx, stream, w - 3, n, fmt, 4096, idx))        # truncated
        expect(zz.E_DATA, lambda: decode(ctx, dev(bytes(raw) + b"\x00"), w + 1, n, fmt, 4096, idx))   # trailing byte
        # too small a destination: an error, and nothing written past cap
        small = n // 2
        out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        expect(zz.E_NOSPACE, lambda: ctx.decode(stream, w, out, small, fmt, 4096, idx))
        assert bool((out[small:] == 0xA5).all())
        out.fill_(0xA5)
        expect(zz.E_NOSPACE, lambda: ctx.decode(stream, w, out, small, fmt, 0, None))
        assert bool((out[small:] == 0xA5).all())
    stream, w = encode(ctx, src, n, 1, 1, 32768)
    raw = bytearray(stream.cpu().numpy().tobytes())
    raw[-4] ^= 1                                                              # ISIZE
    expect(zz.E_DATA, lambda: decode(ctx, dev(bytes(raw)), w, n, 1, 32768, ctx.packet_index()))
    fdict = b"\x78\xbb" + b"\x00" * 8
    assert (0x78 * 256 + 0xBB) % 31 == 0
    expect(zz.E_UNSUPPORTED, lambda: decode(ctx, dev(fdict), len(fdict), 10, 0, 0))


def test_non_first_shard_is_too_far_back(ctx):
    data = synth("period", 200000, 4)
    src = dev(data)
    P = 32768
    half = 3 * P
    cap = zz.bound(len(data), 2, 2, P)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    w, _ = ctx.encode_shard(src[half:], len(data) - half, dst, cap, halo=half, is_last=True, checksum=zz.Format.Deflate,
                            level=2, packet_size=P)
    expect(zz.E_DATA, lambda: decode(ctx, dst[:w].clone(), w, len(data), 2, 0))


def test_garbage_gives_errors(ctx):
    rng = random.Random(5)
    base = zlib.compress(corpus_file("grammar.lsp"), 6)
    cases = [bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 3000))) for _ in range(12)]
    cases += [base[:k] for k in range(0, len(base), max(1, len(base) // 40))]
    for i in range(0, len(base), 7):
        b = bytearray(base); b[i] ^= 1 << (i % 8); cases.append(bytes(b))
    for s in cases:
        for fmt in (0, 1, 2):
            for P in (0, 32768, 1000):
                try:
                    decode(ctx, dev(s), len(s), 8192, fmt, P, slack=0)
                except zz.ZzFlateError as e:
                    assert e.code in (zz.E_DATA, zz.E_NOSPACE, zz.E_UNSUPPORTED)


GIB = 1 << 30


@pytest.mark.parametrize("kind,n,lvl,fmt", [(zz.GEN_TEXT, GIB, 1, 0), (zz.GEN_TEXT, GIB, 2, 0), (zz.GEN_MIX, 2 * GIB, 3, 0),
                                            (zz.GEN_MIX, 2 * GIB, 6, 0), (zz.GEN_LOG, GIB, 2, 1)])
def test_full_size(xctx, kind, n, lvl, fmt):
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    xctx.generate(kind, 1, 0, src, n)
    stream, w = encode(xctx, src, n, fmt, lvl, 32768)
    idx = xctx.packet_index()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    got = xctx.decode(stream, w, out, n, fmt, 32768, idx)
    assert got == n and torch.equal(out, src)
    assert xctx.last_decode_path() == zz.DECODE_INDEXED
    del out, stream, src
    torch.cuda.empty_cache()
