"""The window sidecar of a point index built on the host and built on the device (zz_points_windows_host,
zz_points_windows_device), beside the decode it should cost: one JSON line per stream and sidecar spacing, appended to --out.

    python tools/bench_points_windows.py [--data text|mix ...] [--level 1|6 ...] [--spacing N ...] [--mib 512] [--calls 5]
                                         [--host-calls 5] [--only device] [--out profiles/r17_points_windows_bench.jsonl]

The stream: --mib MiB (a 16 MiB unit of zz_generate_device repeated; for the mix 1 MiB of each of its twelve families in turn)
compressed by host zlib at --level as ONE zlib stream. The dense index is Context.points_index's (chunk 16,384, spacing 1), the
sidecar's rows are points_thin(dense, spacing) for the spacings 32 KiB, 128 KiB and 1 MiB. Per line, in one run and one process,
each the median (min, max) wall time of --calls synchronous calls after one warm-up:
  host_*          zz_points_windows_host (--host-calls calls: it is one core's pass of seconds)
  same_*          the device call decoding with the sidecar's own rows (fine_points NULL)
  fine_*          the device call decoding with the dense rows
  fine_dst_*      the same, also leaving the decoded stream in a destination
  decode_*        decode_points over the dense rows: what the builder's decode costs alone
  open_*          open_found followed by one read of 4 KiB: first contact to first byte
and the two ratios fine_vs_decode (fine_ms / decode_ms) and host_vs_fine (host_ms / fine_ms). The device's sidecar is compared with
the host's on the device after every call, outside the clock; so are the decoded bytes. --only device runs nothing but the fine_*
calls (for a kernel trace of its own).
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
SPACINGS = (32768, 131072, 1048576)
CHUNK = 16384


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


def stream_of(ctx, data, level, mib):
    unit = torch.empty(UNIT, dtype=torch.uint8, device="cuda")
    if data == "mix":
        for j in range(UNIT >> 20):
            ctx.generate(DATA[data], 1, (j % 12) * UNIT + ((j // 12) << 20), unit[j << 20:], 1 << 20)
    else:
        ctx.generate(DATA[data], 1, 0, unit, UNIT)
    reps = max(1, (mib << 20) // UNIT)
    plain = unit.repeat(reps)
    return plain, zlib.compress(plain.cpu().numpy().tobytes(), level)


def run(ctx, data, level, plain, stream, spacing, calls, host_calls, only):
    total = plain.numel()
    src = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    dense, n = ctx.points_index(src, len(stream), zz.Format.Zlib, CHUNK, 1)
    assert n == total
    points = zz.points_thin(dense, spacing)
    line = {"data": data, "level": level, "bytes": total, "stream_bytes": len(stream), "spacing": spacing, "calls": calls,
            "host_calls": host_calls, "dense_rows": dense.shape[0], "rows": points.shape[0]}
    got = {}
    want = {}

    def nothing():
        pass

    def same_sidecar():
        if want:
            assert torch.equal(got["sums"], want["sums"]) and torch.equal(got["windows"], want["windows"])
        got.clear()

    if not only:
        hms = []
        for _ in range(host_calls):
            t = time.perf_counter()
            w, s = zz.points_windows_host(stream, points, zz.Format.Zlib)
            hms.append((time.perf_counter() - t) * 1e3)
        hms.sort()
        line.update(three("host", hms, total))
        want["windows"], want["sums"] = w.cuda(), s.cuda()
        del w, s

    def device(fine, dst):
        def call():
            got["windows"], got["sums"] = ctx.points_windows(src, len(stream), points, zz.Format.Zlib, fine_points=fine, dst=dst, cap=total if dst is not None else None)
        return call

    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")

    def same_all():
        same_sidecar()
        assert torch.equal(out[:total], plain)
        out.zero_()

    line.update(three("fine", wall(device(dense, None), same_sidecar, calls), total))
    line["fine_batches"], line["fine_pending"], line["fine_rounds"] = ctx.last_points_windows_stats()
    if only:
        return line
    line.update(three("same", wall(device(None, None), same_sidecar, calls), total))
    line.update(three("fine_dst", wall(device(dense, out), same_all, calls), total))

    def decode():
        assert ctx.decode_points(src, len(stream), out, total, dense, zz.Format.Zlib) == total

    def decoded():
        assert torch.equal(out[:total], plain)
        out.zero_()

    line.update(three("decode", wall(decode, decoded, calls), total))
    assert ctx.last_decode_path() == zz.DECODE_POINTS
    first = total // 2 + 12345
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def opened():
        p, w, s, length = ctx.open_found(src, len(stream), zz.Format.Zlib, CHUNK, spacing)
        lens, status = ctx.decode_points_ranges(src, len(stream), p, w, s, [first], [4096], [small])
        assert status == [0] and lens == [4096] and length == total
        got["windows"], got["sums"] = w, s

    def read_ok():
        same_sidecar()
        assert torch.equal(small, plain[first: first + 4096])
        small.zero_()

    line.update(three("open", wall(opened, read_ok, calls), total))
    line["fine_vs_decode"] = round(line["fine_ms"] / line["decode_ms"], 3)
    line["host_vs_fine"] = round(line["host_ms"] / line["fine_ms"], 2)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int)
    ap.add_argument("--spacing", action="append", type=int)
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--only", choices=["device"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = zz.Context(0)
    for data in a.data or ["text", "mix"]:
        for level in a.level or [1, 6]:
            plain, stream = stream_of(ctx, data, level, a.mib)
            for spacing in a.spacing or SPACINGS:
                line = json.dumps(run(ctx, data, level, plain, stream, spacing, a.calls, a.host_calls, a.only))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
