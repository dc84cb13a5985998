"""A stream this library did not write, decoded from a point index on one GPU (zz_decode_points_device): one JSON line per
configuration, appended to --out.

    python tools/bench_decode_points.py [--data text|mix ...] [--level 1|6 ...] [--mib 256] [--calls 7] [--only points]
                                        [--spacing N ...] [--out profiles/r14_decode_points_bench.jsonl]

The stream: --mib MiB (a 16 MiB unit of zz_generate_device repeated; for the mix 1 MiB of each of its twelve families in turn)
compressed by host zlib at --level as ONE zlib stream -- what `zlib.compress` or `pigz -p1 -z` leave. Per configuration:
  points_*       per spacing (32 KiB, 128 KiB, 512 KiB): the builder's time and rate over the compressed stream, the segments, the
                 median / min / max wall time of --calls synchronous decode_points calls (after one warm-up; every call's output is
                 compared with the input on the device, outside the clock), decoded GB/s, the pending share and the rounds
  host_zlib_*    zlib.decompress of the same stream on one core
  serial_*       the serial path (decode with packet_size 0) over the first 16 MiB compressed the same way, one call
  packets_*      zz_decode_device with its index over the same bytes written by this library in packet mode at level 1
--only points runs nothing but the decode_points calls (for a kernel trace of its own).
"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402

DATA = {"text": zz.GEN_TEXT, "mix": zz.GEN_MIX}
UNIT = 16 << 20
SPACINGS = (32768, 131072, 524288)


def wall(fn, check, calls):
    """sorted wall times in ms of `calls` synchronous calls, one warm-up in front"""
    fn(); check()
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
        check()
    return sorted(ms)


def run(data, level, mib, calls, only, spacings):
    ctx = zz.Context(0)
    unit = torch.empty(UNIT, dtype=torch.uint8, device="cuda")
    if data == "mix":
        for j in range(UNIT >> 20):
            ctx.generate(DATA[data], 1, (j % 12) * UNIT + ((j // 12) << 20), unit[j << 20:], 1 << 20)
    else:
        ctx.generate(DATA[data], 1, 0, unit, UNIT)
    reps = max(1, (mib << 20) // UNIT)
    total = reps * UNIT
    plain = unit.repeat(reps)
    host = plain.cpu().numpy().tobytes()
    t = time.perf_counter()
    stream = zlib.compress(host, level)
    prep = time.perf_counter() - t
    src = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    line = {"data": data, "level": level, "bytes": total, "stream_bytes": len(stream), "host_compress_s": round(prep, 2), "calls": calls}

    def check():
        assert torch.equal(out[:total], plain)
        out.zero_()

    for spacing in spacings:
        t = time.perf_counter()
        points, n = zz.points_index_host(stream, zz.Format.Zlib, spacing)
        build = time.perf_counter() - t
        assert n == total

        def call():
            assert ctx.decode_points(src, len(stream), out, total, points, zz.Format.Zlib) == total

        ms = wall(call, check, calls)
        assert ctx.last_decode_path() == zz.DECODE_POINTS
        pending, rounds = ctx.last_decode_stats()
        mid = ms[len(ms) // 2]
        k = f"points_{spacing >> 10}k"
        line.update({f"{k}_segments": points.shape[0] - 1, f"{k}_build_ms": round(build * 1e3, 1),
                     f"{k}_build_mbps": round(len(stream) / build / 1e6, 1), f"{k}_build_decoded_mbps": round(total / build / 1e6, 1),
                     f"{k}_ms": round(mid, 3), f"{k}_ms_min": round(ms[0], 3), f"{k}_ms_max": round(ms[-1], 3),
                     f"{k}_gbps": round(total / mid / 1e6, 3), f"{k}_pending_share": round(pending / total, 4), f"{k}_rounds": rounds})
    if only:
        return line
    best = min(line[f"points_{s >> 10}k_ms"] for s in spacings)

    t = time.perf_counter()
    assert len(zlib.decompress(stream)) == total
    hz = (time.perf_counter() - t) * 1e3
    line.update({"host_zlib_ms": round(hz, 1), "host_zlib_gbps": round(total / hz / 1e6, 3), "points_vs_host_zlib": round(hz / best, 2)})

    # the serial path on the first 16 MiB
    small = zlib.compress(host[:UNIT], level)
    ssrc = torch.frombuffer(bytearray(small), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    t = time.perf_counter()
    assert ctx.decode(ssrc, len(small), out, UNIT, zz.Format.Zlib, 0) == UNIT
    torch.cuda.synchronize()
    sms = (time.perf_counter() - t) * 1e3
    assert ctx.last_decode_path() == zz.DECODE_SERIAL and torch.equal(out[:UNIT], unit)
    out.zero_()
    line.update({"serial_bytes": UNIT, "serial_ms": round(sms, 1), "serial_mbps": round(UNIT / sms / 1e3, 2),
                 "points_vs_serial_rate": round((total / best) / (UNIT / sms), 1)})

    # the same bytes written by this library in packet mode, decoded through their packet index
    cap = zz.bound(total, zz.Format.Zlib, 1)
    enc = torch.empty(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(plain, total, enc, cap, zz.Format.Zlib, 1)
    index = ctx.packet_index()

    def packets():
        assert ctx.decode(enc, w, out, total, zz.Format.Zlib, zz.DEFAULT_PACKET, index) == total

    pms = wall(packets, check, calls)
    assert ctx.last_decode_path() == zz.DECODE_INDEXED
    pmid = pms[len(pms) // 2]
    line.update({"packets_ms": round(pmid, 3), "packets_gbps": round(total / pmid / 1e6, 3)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--spacing", action="append", type=int)
    ap.add_argument("--only", choices=["points"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for data in a.data or ["text", "mix"]:
        for level in a.level or [1, 6]:
            line = json.dumps(run(data, level, a.mib, a.calls, a.only, tuple(a.spacing or SPACINGS)))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
