"""What the check costs: checked and unchecked range reads of one large indexed stream beside each other in one process
(zz_decode_range_checked_device against zz_decode_range_device, zz_decode_ranges_checked_device against zz_decode_ranges_device):
one JSON line per configuration.

    python tools/bench_decode_range_checked.py [--case text_l1] [--format zlib] [--gib 1] [--reads 15] [--warmup 2]

The input is generated on the device and encoded with the library (32 KiB packets); the stream, its packet index and its sidecar
(zz_packet_checksums_device of the input) stay in HBM. Single reads of 4 KiB, 1 MiB and 64 MiB at seeded random offsets, and one
multi read of 768 x 4 KiB: every offset is read by the unchecked call and then by the checked call, so both see the same packets in
the same state of the caches and clocks; each result is compared with the input. Reported per length: median, min and max call
time (host clock around the synchronous call) of both, and the ratio of the medians. The unchecked figures are this run's own, not
the ones in README.md. Run under a time limit:

    timeout -k 10 600 python tools/bench_decode_range_checked.py --case text_l1 >> profiles/r13_decode_checked_bench.jsonl
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

CASES = {"text_l1": (zz.GEN_TEXT, 1), "text_l2": (zz.GEN_TEXT, 2)}
FORMATS = {"zlib": zz.Format.Zlib, "gzip": zz.Format.Gzip}
LENGTHS = (4 << 10, 1 << 20, 64 << 20)
MULTI = (768, 4 << 10)
P = 32768


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def stats(ts):
    return {"ms_median": round(1e3 * statistics.median(ts), 3), "ms_min": round(1e3 * min(ts), 3), "ms_max": round(1e3 * max(ts), 3)}


def run(name, fmt_name, gib, reads, warmup):
    kind, lvl = CASES[name]
    fmt = FORMATS[fmt_name]
    n = int(gib * (1 << 30))
    ctx = zz.Context(0)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(kind, 1, 0, src, n)
    cap = zz.bound(n, fmt, lvl, P)
    stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, n, stream, cap, fmt, lvl, P)
    index = ctx.packet_index()
    cks, t_side = timed(lambda: ctx.packet_checksums(src, n, fmt, P))
    cks, t_side = timed(lambda: ctx.packet_checksums(src, n, fmt, P))
    line = {"case": name, "format": fmt_name, "level": lvl, "bytes": n, "stream_bytes": w, "packet_size": P, "packets": index.numel() - 1,
            "reads": reads, "sidecar_ms": round(1e3 * t_side, 3), "ranges": []}
    rng = random.Random(1)
    for length in LENGTHS:
        if length > n:
            continue
        dst = torch.empty(length, dtype=torch.uint8, device="cuda")
        plain, checked = [], []
        for i in range(warmup + reads):
            first = rng.randrange(n - length + 1)
            m0, t0 = timed(lambda: ctx.decode_range(stream, w, dst, length, first, length, fmt, P, index))
            assert m0 == length and torch.equal(dst, src[first: first + length]), f"{name}: range {first}+{length} differs from the input"
            dst.zero_()
            m1, t1 = timed(lambda: ctx.decode_range_checked(stream, w, dst, length, first, length, cks, n, fmt, P, index))
            assert m1 == length and torch.equal(dst, src[first: first + length]), f"{name}: checked range {first}+{length} differs"
            if i >= warmup:
                plain.append(t0); checked.append(t1)
        line["ranges"].append({"nbytes": length, "unchecked": stats(plain), "checked": stats(checked),
                               "checked_over_unchecked": round(statistics.median(checked) / statistics.median(plain), 3)})
    count, length = MULTI
    outs = [torch.empty(length, dtype=torch.uint8, device="cuda") for _ in range(count)]
    plain, checked = [], []
    for i in range(warmup + reads):
        firsts = [rng.randrange(n - length + 1) for _ in range(count)]
        nbytes = [length] * count
        (lens, status), t0 = timed(lambda: ctx.decode_ranges(stream, w, firsts, nbytes, outs, None, fmt, P, index))
        assert status == [0] * count and all(torch.equal(o, src[f: f + length]) for o, f in zip(outs[::97], firsts[::97]))
        (lens, status), t1 = timed(lambda: ctx.decode_ranges_checked(stream, w, firsts, nbytes, outs, cks, n, None, fmt, P, index))
        assert status == [0] * count and all(torch.equal(o, src[f: f + length]) for o, f in zip(outs[::97], firsts[::97]))
        if i >= warmup:
            plain.append(t0); checked.append(t1)
    line["multi"] = {"reads_per_call": count, "nbytes": length, "unchecked": stats(plain), "checked": stats(checked),
                     "checked_over_unchecked": round(statistics.median(checked) / statistics.median(plain), 3)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="text_l1", choices=sorted(CASES))
    ap.add_argument("--format", default="zlib", choices=sorted(FORMATS))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reads", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    run(a.case, a.format, a.gib, a.reads, a.warmup)


if __name__ == "__main__":
    main()
