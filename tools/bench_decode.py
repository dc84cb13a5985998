"""Decode throughput on one GPU (zz_decode_device): one JSON line per case.

    python tools/bench_decode.py [--case NAME ...] [--gib 1] [--steps 5] [--warmup 2] [--no-host]

Inputs are generated on the device (zz_generate_device) and encoded with the library (32 KiB packets); every step decodes
the whole stream and checks its trailer (the call does), timed by the host clock around the synchronous call. A line holds
the decompressed GB/s (median and best over the steps), the path taken, the share of bytes phase 1 left pending and the
pointer-jumping rounds that resolved them, and single-thread host zlib.decompress on the same stream, timed in the same
run. Run each case in a process of its own under a time limit (`timeout -k 10 <s> python tools/bench_decode.py --case X`).
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402

# name: (generator, level, format, index given, packet size for the decode, size divisor)
CASES = {
    "text_l1": (zz.GEN_TEXT, 1, zz.Format.Zlib, True, 32768, 1),
    "text_l2": (zz.GEN_TEXT, 2, zz.Format.Zlib, True, 32768, 1),
    "mix_l3": (zz.GEN_MIX, 3, zz.Format.Zlib, True, 32768, 1),
    "logs_l2_gzip": (zz.GEN_LOG, 2, zz.Format.Gzip, True, 32768, 1),
    "mix_l6": (zz.GEN_MIX, 6, zz.Format.Zlib, True, 32768, 1),
    "text_l1_discovered": (zz.GEN_TEXT, 1, zz.Format.Zlib, False, 32768, 1),
    "text_l2_discovered": (zz.GEN_TEXT, 2, zz.Format.Zlib, False, 32768, 1),
    "text_l1_serial": (zz.GEN_TEXT, 1, zz.Format.Zlib, False, 0, 64),     # the compatibility path, on 1/64 of the size
}
PATHS = {1: "indexed", 2: "discovered", 3: "serial"}


def run(name, gib, steps, warmup, host):
    kind, lvl, fmt, with_index, P, div = CASES[name]
    n = int(gib * (1 << 30)) // div
    ctx = zz.Context(0)
    ctx.set_extended_levels(True)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(kind, 1, 0, src, n)
    cap = zz.bound(n, fmt, min(lvl, 3), 32768)
    stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, n, stream, cap, fmt, lvl, 32768)
    index = ctx.packet_index() if with_index else None
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ctx.decode(stream, w, out, n, fmt, P, index)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    assert got == n and torch.equal(out, src), f"{name}: the decoded bytes differ from the input"
    pend, rounds = ctx.last_decode_stats()
    line = {
        "case": name, "level": lvl, "format": fmt.name.lower(), "bytes": n, "stream_bytes": w, "packet_size": P,
        "index_given": with_index, "path": PATHS.get(ctx.last_decode_path(), "none"),
        "gbps_median": round(n / statistics.median(times) / 1e9, 2), "gbps_best": round(n / min(times) / 1e9, 2),
        "ms_median": round(1e3 * statistics.median(times), 3), "steps": steps,
        "pending_share": round(pend / n, 6), "pending_bytes": pend, "rounds": rounds,
    }
    if host:
        blob = stream[:w].cpu().numpy().tobytes()
        wbits = 31 if fmt == zz.Format.Gzip else 15
        t0 = time.perf_counter()
        h = zlib.decompress(blob, wbits)
        dt = time.perf_counter() - t0
        assert len(h) == n
        line["host_zlib_1thread_gbps"] = round(n / dt / 1e9, 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    for name in a.case or list(CASES):
        run(name, a.gib, a.steps, a.warmup, not a.no_host)


if __name__ == "__main__":
    main()
