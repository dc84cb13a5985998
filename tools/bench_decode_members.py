"""A blocked (BGZF) gzip file on one GPU (zz_decode_members_device): one JSON line per configuration.

    python tools/bench_decode_members.py [--data text|mix ...] [--level 1|6 ...] [--gib 1] [--min-seconds 1] [--only members]

The file: about --gib GiB of decoded bytes as blocked members of 65,280 input bytes each (the size bgzip cuts), made from a
16 MiB unit (zz_generate_device; for the mix 1 MiB of each of its twelve families in turn) that host zlib compresses member by member; the unit's members are repeated -- members are
independent, so the repetition is a legal file. Per configuration:
  members_ms   the median time of one decode_members call over the file (HIP events on the launch stream, after a warm-up,
               repeated until --min-seconds of timed work); every timed call is followed, outside the clock, by a device
               comparison of the output with the input. members_gbps is DECODED GB/s.
  batch_ms     (a) zz_decode_batch_device over the same members with descriptors made on the host: the bound for what the call
               can reach
  serial_ms    (b) the serial path on the first 16 MiB (the same members without their BC subfield), one call
  hop_ms       the file with one false header (a last member that stores a small blocked file): path 2, the chain walked by
               one lane, one call after a warm-up
--only members runs nothing but the timed call (for a kernel trace of its own).
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402
from bench_decode_batch import timed  # noqa: E402

DATA = {"text": zz.GEN_TEXT, "mix": zz.GEN_MIX}
UNIT = 16 << 20
CUT = 65280


def gz_member(data, level, bc):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush() + struct.pack("<II", zlib.crc32(data), len(data))
    if not bc:
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + body
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(body) - 1) + body


def run(data, level, gib, min_seconds, only):
    ctx = zz.Context(0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    unit = torch.empty(UNIT, dtype=torch.uint8, device="cuda")
    if data == "mix":
        # the generator's mix cycles through twelve families in segments of 16 MiB: the unit takes 1 MiB of each in turn
        for j in range(UNIT >> 20):
            ctx.generate(DATA[data], 1, (j % 12) * UNIT + ((j // 12) << 20), unit[j << 20:], 1 << 20)
    else:
        ctx.generate(DATA[data], 1, 0, unit, UNIT)
    host = unit.cpu().numpy().tobytes()
    parts = [host[i:i + CUT] for i in range(0, UNIT, CUT)]
    ms_bc = [gz_member(p, level, True) for p in parts]
    reps = max(1, round(gib * (1 << 30) / UNIT))
    total = reps * UNIT
    ufile = b"".join(ms_bc)
    file = torch.frombuffer(bytearray(ufile), dtype=torch.uint8).cuda().repeat(reps)
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    got = ctypes.c_uint64(0)

    def members(src=file, n=None, cap=total):
        rc = zz.lib.zz_decode_members_device(ctx._h, src.data_ptr(), src.numel() if n is None else n, out.data_ptr(), cap, ctypes.byref(got), st)
        assert rc == 0, zz.lib.zz_last_error()

    def check():
        assert got.value == total and bool((out[:total].view(reps, UNIT) == unit).all())
        out.zero_()

    ms = timed(members, check, min_seconds, stream)
    mid = ms[len(ms) // 2]
    stats = ctx.last_decode_members_stats()
    assert stats[2] == zz.MEMBERS_BLOCKED and stats[0] == reps * len(parts)
    line = {"data": data, "level": level, "bytes": total, "file_bytes": file.numel(), "members": stats[0], "candidates": stats[1],
            "members_ms": round(mid, 3), "members_ms_min": round(ms[0], 3), "members_ms_max": round(ms[-1], 3), "members_reps": len(ms),
            "members_gbps": round(total / mid / 1e6, 3)}
    if not only:
        # (a) the same members through zz_decode_batch_device, descriptors made on the host
        k = reps * len(parts)
        clen = torch.tensor([len(m) for m in ms_bc] * reps, dtype=torch.int64)
        dlen = torch.tensor([len(p) for p in parts] * reps, dtype=torch.int64)
        srcs = (file.data_ptr() + torch.cumsum(clen, 0) - clen).cuda()
        dsts = (out.data_ptr() + torch.cumsum(dlen, 0) - dlen).cuda()
        clen, dlen = clen.cuda(), dlen.cuda()
        olens = torch.zeros(k, dtype=torch.int64, device="cuda")

        def batch():
            rc = zz.lib.zz_decode_batch_device(ctx._h, k, srcs.data_ptr(), clen.data_ptr(), dsts.data_ptr(), dlen.data_ptr(), olens.data_ptr(),
                                               None, int(zz.Format.Gzip), st)
            assert rc == 0, zz.lib.zz_last_error()

        def check_batch():
            assert bool((out[:total].view(reps, UNIT) == unit).all()) and torch.equal(olens, dlen)
            out.zero_()

        msb = timed(batch, check_batch, min_seconds, stream)
        bmid = msb[len(msb) // 2]
        line.update({"batch_ms": round(bmid, 3), "batch_gbps": round(total / bmid / 1e6, 3), "members_vs_batch": round(mid / bmid, 3)})

        # (b) the serial path on the first 16 MiB
        plain = torch.frombuffer(bytearray(b"".join(gz_member(p, level, False) for p in parts)), dtype=torch.uint8).cuda()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        members(plain, cap=UNIT)
        e1.record(stream)
        e1.synchronize()
        assert got.value == UNIT and torch.equal(out[:UNIT], unit) and ctx.last_decode_members_stats()[2] == zz.MEMBERS_SERIAL
        sms = e0.elapsed_time(e1)
        line.update({"serial_ms": round(sms, 1), "serial_mbps": round(UNIT / sms / 1e3, 2)})

        # the hop: one false header, in a last member that stores a small blocked file
        small = gz_member(b"a member inside a member", 6, True)
        hopf = torch.cat([file, torch.frombuffer(bytearray(gz_member(small, 0, True)), dtype=torch.uint8).cuda()])
        members(hopf, cap=total + len(small))
        torch.cuda.synchronize()
        e0.record(stream)
        members(hopf, cap=total + len(small))
        e1.record(stream)
        e1.synchronize()
        hstats = ctx.last_decode_members_stats()
        assert got.value == total + len(small) and bool((out[:total].view(reps, UNIT) == unit).all())
        assert hstats[2] == zz.MEMBERS_WALKED and hstats[1] > hstats[0]
        line.update({"hop_ms": round(e0.elapsed_time(e1), 3), "hop_members": hstats[0]})
    print(json.dumps(line), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int, choices=list(range(10)))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", choices=["members"])
    a = ap.parse_args()
    for data in a.data or ["text", "mix"]:
        for level in a.level or [1, 6]:
            run(data, level, a.gib, a.min_seconds, a.only)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
