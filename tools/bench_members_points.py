"""A file of gzip members, large or small, through its member point index on one GPU (zz_members_points_device,
zz_decode_members_points_device): one JSON line per configuration.

    python tools/bench_members_points.py [--data text|mix ...] [--level 1|6 ...] [--layout two|loguniform|64k ...] [--gib 1]
                                         [--min-seconds 1] [--only index|decode] [--out FILE]

The file: about --gib GiB of decoded bytes as plain members (ten-byte headers, no `BC`), made from a 16 MiB unit
(zz_generate_device; for the mix 1 MiB of each of its twelve families in turn) that host zlib compresses. Layouts:
  two         two members of half the bytes each (the unit repeated inside one member): `cat lane1.fq.gz lane2.fq.gz`
  loguniform  member sizes drawn log-uniformly from 1 KiB to 1 MiB, the unit's members repeated
  64k         members of 65,280 input bytes, the unit's members repeated
Per configuration, medians of at least three calls after a warm-up (HIP events on the launch stream, repeated until --min-seconds of
timed work), every timed decode followed, outside the clock, by a device comparison with the input:
  index_ms    members_points over the file (default chunk, spacing 1), with its stats
  decode_ms   decode_members_points over the file with those rows; decode_gbps is DECODED GB/s; with its stats
  found_ms    decode_members_found on the same file, measured beside it (layout two: ONE call, no warm-up -- a member is that
              call's unit, so two wavefronts decode the whole file); points_vs_found = found_ms / decode_ms
  serial_ms   decode_members on a 16 MiB prefix written as one member: the serial path
--only index / decode runs nothing but that timed call (for a kernel trace of its own). --out appends the lines to FILE.
"""
import argparse
import ctypes
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402
from bench_decode_batch import timed  # noqa: E402
from bench_decode_members import CUT, DATA, UNIT, gz_member  # noqa: E402
from bench_members_find import cuts  # noqa: E402


def big_member(host, reps, level):
    """one gzip member that holds `host` reps times"""
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    parts = [co.compress(host) for _ in range(reps)]
    parts.append(co.flush())
    return b"".join(parts)


def run(data, level, layout, gib, min_seconds, only, out_path):
    ctx = zz.Context(0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    unit = torch.empty(UNIT, dtype=torch.uint8, device="cuda")
    if data == "mix":
        for j in range(UNIT >> 20):
            ctx.generate(DATA[data], 1, (j % 12) * UNIT + ((j // 12) << 20), unit[j << 20:], 1 << 20)
    else:
        ctx.generate(DATA[data], 1, 0, unit, UNIT)
    host = unit.cpu().numpy().tobytes()
    reps = max(2, round(gib * (1 << 30) / UNIT))
    if layout == "two":
        reps -= reps % 2
        one = torch.frombuffer(bytearray(big_member(host, reps // 2, level)), dtype=torch.uint8).cuda()
        file, members = one.repeat(2), 2
    else:
        sizes = cuts("64k" if layout == "64k" else "loguniform")
        mlist, at = [], 0
        for n in sizes:
            mlist.append(gz_member(host[at:at + n], level, False)); at += n
        file = torch.frombuffer(bytearray(b"".join(mlist)), dtype=torch.uint8).cuda().repeat(reps)
        members = reps * len(sizes)
    total = reps * UNIT
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    got = ctypes.c_uint64(0)
    box = {}

    def index():
        box["rows"], box["n"] = ctx.members_points(file)

    def check_index():
        assert box["n"] == total and ctx.last_members_points_stats()[0] == members

    def decode():
        rows = box["rows"]
        rc = zz.lib.zz_decode_members_points_device(ctx._h, file.data_ptr(), file.numel(), out.data_ptr(), total, ctypes.byref(got), rows.data_ptr(),
                                                    rows.shape[0], 0, st)
        assert rc == 0, zz.lib.zz_last_error()

    def found():
        rc = zz.lib.zz_decode_members_found_device(ctx._h, file.data_ptr(), file.numel(), out.data_ptr(), total, ctypes.byref(got), st)
        assert rc == 0, zz.lib.zz_last_error()

    def check():
        assert got.value == total and bool((out[:total].view(reps, UNIT) == unit).all())
        out.zero_()

    line = {"data": data, "level": level, "layout": layout, "bytes": total, "file_bytes": file.numel(), "members": members}
    index()
    check_index()
    line["rows"] = int(box["rows"].shape[0])
    if only != "decode":
        ms = timed(index, check_index, min_seconds, stream)
        mid = ms[len(ms) // 2]
        _, hc, bc, dropped, rounds = ctx.last_members_points_stats()
        line.update({"header_candidates": hc, "block_candidates": bc, "dropped": dropped, "index_rounds": rounds, "index_ms": round(mid, 3),
                     "index_ms_min": round(ms[0], 3), "index_ms_max": round(ms[-1], 3), "index_reps": len(ms), "index_gbps": round(total / mid / 1e6, 3)})
    if only != "index":
        ms = timed(decode, check, min_seconds, stream)
        mid = ms[len(ms) // 2]
        m, proven, segs, batches, pending, rounds, serial = ctx.last_decode_members_points_stats()
        assert (m, proven, serial) == (members, members, 0), (m, proven, serial)
        line.update({"decode_ms": round(mid, 3), "decode_ms_min": round(ms[0], 3), "decode_ms_max": round(ms[-1], 3), "decode_reps": len(ms),
                     "decode_gbps": round(total / mid / 1e6, 3), "segments": segs, "batches": batches, "pending_share": round(pending / total, 3),
                     "rounds": rounds})
    if not only:
        if layout == "two":                                       # two wavefronts over the whole file: one call is a minute or more
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            found()
            e1.record(stream)
            e1.synchronize()
            check()
            fmid, freps = e0.elapsed_time(e1), 1
        else:
            ms = timed(found, check, min_seconds, stream)
            fmid, freps = ms[len(ms) // 2], len(ms)
        line.update({"found_ms": round(fmid, 3), "found_reps": freps, "found_gbps": round(total / fmid / 1e6, 3),
                     "points_vs_found": round(fmid / line["decode_ms"], 2)})
        # the serial path over a 16 MiB prefix, one call
        prefix = torch.frombuffer(bytearray(big_member(host, 1, level)), dtype=torch.uint8).cuda()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = zz.lib.zz_decode_members_device(ctx._h, prefix.data_ptr(), prefix.numel(), out.data_ptr(), UNIT, ctypes.byref(got), st)
        e1.record(stream)
        e1.synchronize()
        assert rc == 0 and got.value == UNIT and torch.equal(out[:UNIT], unit) and ctx.last_decode_members_stats()[2] == zz.MEMBERS_SERIAL
        sms = e0.elapsed_time(e1)
        line.update({"serial_ms": round(sms, 1), "serial_mbps": round(UNIT / sms / 1e3, 2),
                     "points_vs_serial": round((total / line["decode_ms"]) / (UNIT / sms), 1)})
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        with open(out_path, "a") as fh:
            fh.write(text + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int, choices=list(range(10)))
    ap.add_argument("--layout", action="append", choices=["two", "loguniform", "64k"])
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", choices=["index", "decode"])
    ap.add_argument("--out")
    a = ap.parse_args()
    for layout in a.layout or ["two", "loguniform", "64k"]:
        for data in a.data or ["text", "mix"]:
            for level in a.level or [1, 6]:
                run(data, level, layout, a.gib, a.min_seconds, a.only, a.out)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
