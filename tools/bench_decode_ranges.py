"""Many small reads of a large indexed stream in one call (zz_decode_ranges_device) beside one zz_decode_range_device call per
read: one JSON line per configuration.

    python tools/bench_decode_ranges.py [--gib 1] [--calls 5] [--seconds 240]      # every configuration, a process each
    python tools/bench_decode_ranges.py --case text_l1 [--only 768]                # one configuration, in this process

Without --case the tool starts one process per configuration (1 GiB of level-1 text, of level-2 text; 32 KiB packets), each under
its own `timeout`, and stops at the first that fails. A configuration generates its input on the device, encodes it with the
library and, for N = 1, 64, 768, 4,096 and 65,536 reads of 4 KiB at seeded random offsets, times ONE call for all N (host clock
around the synchronous call, the median of `calls` calls) and, in the same process, the first min(N, 200) of the same reads as one
zz_decode_range_device call each (the median single call; N of them would take N times that). Every read of every timed call is
compared with the input, outside the clock. `ratio` is N single calls at their median over the one call.

--only N times nothing but the one call for N reads, `calls` times: the form to run under `rocprofv3 --kernel-trace --stats --`,
whose sum of kernel times, over `calls`, stands beside the printed call time."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"text_l1": 1, "text_l2": 2}
COUNTS = (1, 64, 768, 4096, 65536)
READ = 4 << 10
P = 32768


def run(name, gib, calls, only):
    import torch
    import zzflate_amd as zz
    lvl = CASES[name]
    n = int(gib * (1 << 30))
    ctx = zz.Context(0)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 1, 0, src, n)
    cap = zz.bound(n, zz.Format.Zlib, lvl, P)
    stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
    w = ctx.encode(src, n, stream, cap, zz.Format.Zlib, lvl, P)
    index = ctx.packet_index()
    rng = random.Random(1)
    firsts = [rng.randrange(n - READ + 1) for _ in range(max(COUNTS))]
    want_at = torch.tensor(firsts, dtype=torch.int64, device="cuda")
    dst = torch.empty(max(COUNTS) * READ, dtype=torch.uint8, device="cuda")
    line = {"case": name, "level": lvl, "bytes": n, "stream_bytes": w, "packet_size": P, "read_bytes": READ, "calls": calls, "counts": []}
    for N in (COUNTS if only is None else (only,)):
        # the six device arrays are made once, outside the clock: the C call is what is timed
        tab = torch.tensor([firsts[:N], [READ] * N, [dst.data_ptr() + i * READ for i in range(N)], [READ] * N], dtype=torch.int64).cuda()
        lens = torch.empty(N, dtype=torch.int64, device="cuda")
        status = torch.empty(N, dtype=torch.int32, device="cuda")
        st = ctx._stream()
        want = src[(want_at[:N, None] + torch.arange(READ, device="cuda")[None, :]).reshape(-1)]
        times = []
        for i in range(calls + 1):                             # the first call grows the workspace and is not counted
            dst[: N * READ].zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = zz.lib.zz_decode_ranges_device(ctx._h, stream.data_ptr(), w, int(zz.Format.Zlib), P, index.data_ptr(), index.numel(), N,
                                                tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(),
                                                lens.data_ptr(), status.data_ptr(), st)
            dt = time.perf_counter() - t0
            assert rc == 0 and not bool(status.any()) and bool((lens == READ).all()), f"{name}: {N} reads: {zz.lib.zz_last_error().decode()}"
            assert torch.equal(dst[: N * READ], want), f"{name}: a read of {N} differs from the input"
            if i:
                times.append(dt)
        packets, attempts, retried, waves = ctx.last_decode_ranges_stats()
        entry = {"reads": N, "call_ms_median": round(1e3 * statistics.median(times), 3), "call_ms_best": round(1e3 * min(times), 3),
                 "reads_per_second": round(N / statistics.median(times)), "stage_packets": packets, "attempts": attempts,
                 "retried_reads": retried, "waves": waves}
        if only is None:
            one = torch.empty(READ, dtype=torch.uint8, device="cuda")
            singles = []
            for i in range(min(N, 200) + 1):
                f = firsts[i % N]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = ctx.decode_range(stream, w, one, READ, f, READ, zz.Format.Zlib, P, index)
                dt = time.perf_counter() - t0
                assert m == READ and torch.equal(one, src[f: f + READ]), f"{name}: single read at {f} differs from the input"
                if i:
                    singles.append(dt)
            ms = statistics.median(singles)
            entry.update({"single_call_ms_median": round(1e3 * ms, 3), "single_reads_per_second": round(1 / ms),
                          "ratio": round(N * ms / statistics.median(times), 1)})
        line["counts"].append(entry)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", type=int)
    ap.add_argument("--seconds", type=int, default=240, help="time limit of one configuration's process")
    a = ap.parse_args()
    if a.calls < 5:
        ap.error("--calls must be at least 5")
    if a.case:
        run(a.case, a.gib, a.calls, a.only)
        return
    for name in CASES:
        r = subprocess.run(["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--gib", str(a.gib), "--calls", str(a.calls)])
        if r.returncode:
            sys.exit(f"{name}: exit status {r.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
