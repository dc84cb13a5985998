"""The point index of a stream this library did not write, built on the host and built on the device (zz_points_index_host,
zz_points_index_device), and the decode with each: one JSON line per configuration, appended to --out.

    python tools/bench_points_index.py [--data text|mix ...] [--level 1|6 ...] [--mib 512] [--calls 5] [--only device]
                                       [--chunk N ...] [--out profiles/r16_points_index_bench.jsonl]

The stream: --mib MiB (a 16 MiB unit of zz_generate_device repeated; for the mix 1 MiB of each of its twelve families in turn)
compressed by host zlib at --level as ONE zlib stream. Per configuration, in the same run:
  host_*          zz_points_index_host at spacing 32,768: one pass on one core; its time, its rate over the decoded bytes, its rows,
                  and decode_points with that index
  device_<C>_*    zz_points_index_device at chunk_bytes C (16,384 and its two neighbours 8,192 and 32,768), spacing 1: median / min /
                  max wall time of --calls synchronous calls after one warm-up, the rate over the decoded bytes, the rows, the
                  candidates, the dropped candidates and the rounds; then decode_points with that index
  found_*         decode_found at chunk 16,384 end to end (index and decode), against zlib.decompress on one core
Every decode's output is compared with the input on the device, outside the clock. --only device runs nothing but the
zz_points_index_device calls (for a kernel trace of its own).
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
CHUNKS = (8192, 16384, 32768)
HOST_SPACING = 32768


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


def three(prefix, ms, total):
    mid = ms[len(ms) // 2]
    return {f"{prefix}_ms": round(mid, 3), f"{prefix}_ms_min": round(ms[0], 3), f"{prefix}_ms_max": round(ms[-1], 3),
            f"{prefix}_gbps": round(total / mid / 1e6, 3)}


def run(data, level, mib, calls, only, chunks):
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
    stream = zlib.compress(host, level)
    src = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    line = {"data": data, "level": level, "bytes": total, "stream_bytes": len(stream), "calls": calls}

    def check():
        assert torch.equal(out[:total], plain)
        out.zero_()

    def nothing():
        pass

    def decode_with(points, prefix):
        def call():
            assert ctx.decode_points(src, len(stream), out, total, points, zz.Format.Zlib) == total
        ms = wall(call, check, calls)
        assert ctx.last_decode_path() == zz.DECODE_POINTS
        line.update(three(prefix, ms, total))
        line[f"{prefix}_rounds"] = ctx.last_decode_stats()[1]

    for chunk in chunks:
        got = {}

        def build():
            got["points"], got["n"] = ctx.points_index(src, len(stream), zz.Format.Zlib, chunk)

        ms = wall(build, nothing, calls)
        assert got["n"] == total
        cand, dropped, rounds = ctx.last_points_index_stats()
        k = f"device_{chunk >> 10}k"
        line.update(three(f"{k}_index", ms, total))
        line.update({f"{k}_rows": got["points"].shape[0], f"{k}_candidates": cand, f"{k}_dropped": dropped, f"{k}_rounds": rounds})
        if not only:
            decode_with(got["points"], f"{k}_decode")
    if only:
        return line

    t = time.perf_counter()
    points, n = zz.points_index_host(stream, zz.Format.Zlib, HOST_SPACING)
    hb = (time.perf_counter() - t) * 1e3
    assert n == total
    line.update({"host_index_ms": round(hb, 1), "host_index_gbps": round(total / hb / 1e6, 3), "host_rows": points.shape[0]})
    decode_with(points, "host_decode")

    def found():
        assert ctx.decode_found(src, len(stream), out, total, zz.Format.Zlib, 16384) == total

    line.update(three("found", wall(found, check, calls), total))
    t = time.perf_counter()
    assert len(zlib.decompress(stream)) == total
    hz = (time.perf_counter() - t) * 1e3
    line.update({"host_zlib_ms": round(hz, 1), "host_zlib_gbps": round(total / hz / 1e6, 3), "found_vs_host_zlib": round(hz / line["found_ms"], 2),
                 "device_index_vs_host_index": round(hb / line["device_16k_index_ms"], 2) if "device_16k_index_ms" in line else None})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int)
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chunk", action="append", type=int)
    ap.add_argument("--only", choices=["device"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for data in a.data or ["text", "mix"]:
        for level in a.level or [1, 6]:
            line = json.dumps(run(data, level, a.mib, a.calls, a.only, tuple(a.chunk or CHUNKS)))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
