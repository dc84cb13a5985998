"""Range reads from a large indexed stream on one GPU (zz_decode_range_device): one JSON line per configuration.

    python tools/bench_decode_range.py --case text_l1 [--gib 1] [--reads 15] [--warmup 2]

The input is generated on the device and encoded with the library (32 KiB packets); the stream and its packet index stay in
HBM. For each range length (4 KiB, 1 MiB, 64 MiB) the tool reads `reads` ranges at seeded random offsets, each checked against
the input, and reports the median and best call time (host clock around the synchronous call), the packets decoded and the
attempts (median and maximum over the reads) -- beside zz_decode_device of the whole stream, timed in the same run. Run each
configuration in a process of its own under a time limit:

    for c in text_l1 text_l2 mix_l6; do timeout -k 10 300 python tools/bench_decode_range.py --case $c || break; done
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402

CASES = {"text_l1": (zz.GEN_TEXT, 1), "text_l2": (zz.GEN_TEXT, 2), "mix_l6": (zz.GEN_MIX, 6)}
LENGTHS = (4 << 10, 1 << 20, 64 << 20)
P = 32768


def run(name, gib, reads, warmup):
    kind, lvl = CASES[name]
    n = int(gib * (1 << 30))
    ctx = zz.Context(0)
    ctx.set_extended_levels(True)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(kind, 1, 0, src, n)
    cap = zz.bound(n, zz.Format.Zlib, min(lvl, 3), P)
    stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, n, stream, cap, zz.Format.Zlib, lvl, P)
    index = ctx.packet_index()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    whole = []
    for i in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ctx.decode(stream, w, out, n, zz.Format.Zlib, P, index)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    assert got == n
    line = {"case": name, "level": lvl, "bytes": n, "stream_bytes": w, "packet_size": P, "reads": reads,
            "whole_stream_ms": round(1e3 * min(whole[1:]), 3), "whole_stream_gbps": round(n / min(whole[1:]) / 1e9, 2), "ranges": []}
    rng = random.Random(1)
    for length in LENGTHS:
        if length > n:
            continue
        dst = torch.empty(length, dtype=torch.uint8, device="cuda")
        times, packets, attempts = [], [], []
        for i in range(warmup + reads):
            first = rng.randrange(n - length + 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = ctx.decode_range(stream, w, dst, length, first, length, zz.Format.Zlib, P, index)
            dt = time.perf_counter() - t0
            assert m == length and torch.equal(dst, src[first: first + length]), f"{name}: range {first}+{length} differs from the input"
            if i >= warmup:
                _, npk, tries, _ = ctx.last_decode_range_stats()
                times.append(dt); packets.append(npk); attempts.append(tries)
        line["ranges"].append({
            "nbytes": length, "ms_median": round(1e3 * statistics.median(times), 3), "ms_best": round(1e3 * min(times), 3),
            "gbps_median": round(length / statistics.median(times) / 1e9, 3),
            "packets_median": statistics.median(packets), "packets_max": max(packets),
            "attempts_median": statistics.median(attempts), "attempts_max": max(attempts),
            "speedup_over_whole_stream": round(min(whole[1:]) / statistics.median(times), 1)})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reads", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    run(a.case, a.gib, a.reads, a.warmup)


if __name__ == "__main__":
    main()
