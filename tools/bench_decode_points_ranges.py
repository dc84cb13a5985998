"""Reads of a stream this library did not write through a point index with windows, on one GPU
(zz_decode_points_ranges_device): one JSON line per row, appended to --out.

    python tools/bench_decode_points_ranges.py [--data text|mix ...] [--level 1|6 ...] [--mib 512] [--calls 7] [--spacing N ...]
                                               [--reads N ...] [--out profiles/r15_decode_points_ranges_bench.jsonl]

The stream is tools/bench_decode_points.py's: --mib MiB (a 16 MiB unit of zz_generate_device repeated; for the mix 1 MiB of each
of its twelve families in turn) compressed by host zlib at --level as ONE zlib stream. Per stream and spacing (32 KiB, 128 KiB,
1 MiB):
  sidecar        the two host passes: zz_points_index_host and zz_points_windows_host, their times and rates, the sidecar's bytes
  whole          the median zz_decode_points_device call over the whole stream through the same index: what a reader pays today
                 for any read, measured beside the reads in this process
  reads          one row per count (1, 64, 768, 4,096): the median call with that many seeded 4 KiB reads at random offsets;
                 `vs_whole` is its time over the `whole` row's
  one 64 MiB read
Times are wall-clock around synchronous calls, after one warm-up: the median of --calls, min and max kept. Every call's bytes are
compared with the input on the device, outside the clock.
"""
import argparse
import json
import os
import random
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402
from bench_decode_points import DATA, UNIT, wall  # noqa: E402

READ = 4096
SPACINGS = (32768, 131072, 1048576)


def summary(ms):
    return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}


def run(data, level, mib, calls, spacings, counts, emit):
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
    stream = zlib.compress(plain.cpu().numpy().tobytes(), level)
    src = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    base = {"data": data, "level": level, "bytes": total, "stream_bytes": len(stream), "calls": calls}

    for spacing in spacings:
        t = time.perf_counter()
        points, n = zz.points_index_host(stream, zz.Format.Zlib, spacing)
        t_index = time.perf_counter() - t
        assert n == total
        t = time.perf_counter()
        windows, sums = zz.points_windows_host(stream, points, zz.Format.Zlib)
        t_win = time.perf_counter() - t
        segments = points.shape[0] - 1
        here = {**base, "spacing": spacing, "segments": segments}
        emit({**here, "row": "sidecar", "index_ms": round(t_index * 1e3, 1), "windows_ms": round(t_win * 1e3, 1),
              "windows_decoded_mbps": round(total / t_win / 1e6, 1), "sidecar_bytes": segments * (zz.POINTS_WINDOW + 4),
              "sidecar_share": round(segments * (zz.POINTS_WINDOW + 4) / total, 4)})
        d_points, d_windows, d_sums = points.cuda(), windows.cuda(), sums.cuda()

        def whole():
            assert ctx.decode_points(src, len(stream), out, total, points, zz.Format.Zlib) == total

        def check_whole():
            assert torch.equal(out[:total], plain)
            out.zero_()

        ms = wall(whole, check_whole, calls)
        whole_ms = ms[len(ms) // 2]
        emit({**here, "row": "whole", **summary(ms), "gbps": round(total / whole_ms / 1e6, 3)})

        def reads_row(name, firsts, nbytes):
            k = len(firsts)
            offs = [0]
            for nb in nbytes:
                offs.append(offs[-1] + nb)
            tab = torch.tensor([firsts, nbytes, [out.data_ptr() + o for o in offs[:-1]], nbytes], dtype=torch.int64).cuda()
            lens = torch.zeros(k, dtype=torch.int64, device="cuda")
            status = torch.zeros(k, dtype=torch.int32, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def call():
                rc = zz.lib.zz_decode_points_ranges_device(ctx._h, src.data_ptr(), len(stream), int(zz.Format.Zlib), d_points.data_ptr(),
                                                           d_points.shape[0], d_windows.data_ptr(), d_sums.data_ptr(), k, tab[0].data_ptr(),
                                                           tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), lens.data_ptr(),
                                                           status.data_ptr(), st)
                assert rc == 0, zz.lib.zz_last_error()

            def check():
                assert bool((status == 0).all()) and torch.equal(lens, tab[1])
                for a, nb, o in zip(firsts, nbytes, offs):
                    assert torch.equal(out[o:o + nb], plain[a:a + nb]), (name, a)
                out[:offs[-1]].zero_()

            ms = wall(call, check, calls)
            dec, waves = ctx.last_decode_points_ranges_stats()
            emit({**here, "row": name, "reads": k, "read_bytes": offs[-1], **summary(ms), "segments_decoded": dec, "waves": waves,
                  "vs_whole": round(ms[len(ms) // 2] / whole_ms, 3)})

        rng = random.Random(12)
        for k in counts:
            reads_row("reads", [rng.randrange(total - READ) for _ in range(k)], [READ] * k)
        big = min(64 << 20, total // 2)
        reads_row("one 64 MiB read", [rng.randrange(total - big)], [big])
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int)
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--spacing", action="append", type=int)
    ap.add_argument("--reads", action="append", type=int)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    for data in a.data or ["text", "mix"]:
        for level in a.level or [1, 6]:
            run(data, level, a.mib, a.calls, tuple(a.spacing or SPACINGS), a.reads or [1, 64, 768, 4096], emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
