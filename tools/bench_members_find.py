"""A file of gzip members that announce no length, on one GPU (zz_members_find_device, zz_decode_members_found_device): one JSON
line per configuration.

    python tools/bench_members_find.py [--data text|mix ...] [--level 1|6 ...] [--layout 64k|loguniform ...] [--gib 1]
                                       [--min-seconds 1] [--only find|found]

The file: about --gib GiB of decoded bytes as plain members (ten-byte headers, no `BC`), made from a 16 MiB unit
(zz_generate_device; for the mix 1 MiB of each of its twelve families in turn) that host zlib compresses member by member; the
unit's members are repeated -- members are independent, so the repetition is a legal file. Layouts: 64k = members of 65,280 input
bytes (the size bgzip cuts, so that the blocked file below holds the same members); loguniform = member sizes drawn log-uniformly
from 1 KiB to 1 MiB. Per configuration, medians of at least three calls after a warm-up (HIP events on the launch stream, repeated
until --min-seconds of timed work), every timed decode followed, outside the clock, by a device comparison with the input:
  find_ms     members_find over the file: mark, measure, walk, index rows
  found_ms    decode_members_found over the file; found_gbps is DECODED GB/s
  serial_ms   decode_members on the first 16 MiB of the same file: the serial path, what the library did for such a file before
  blocked_ms  decode_members on the same bytes rewritten as BGZF (members of 65,280 input bytes with `BC`): the upper bound
  zlib_ms     zlib's member loop over the first 16 MiB on one core
--only find / found runs nothing but that timed call (for a kernel trace of its own).
"""
import argparse
import ctypes
import json
import math
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
from bench_decode_batch import timed  # noqa: E402
from bench_decode_members import CUT, DATA, UNIT, gz_member  # noqa: E402


def cuts(layout):
    """the unit's member sizes"""
    if layout == "64k":
        return [min(CUT, UNIT - i) for i in range(0, UNIT, CUT)]
    rng, sizes, left = random.Random(7), [], UNIT
    while left:
        n = min(left, int(math.exp(rng.uniform(math.log(1 << 10), math.log(1 << 20)))))
        sizes.append(n); left -= n
    return sizes


def run(data, level, layout, gib, min_seconds, only):
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
    sizes, parts, at = cuts(layout), [], 0
    for n in sizes:
        parts.append(host[at:at + n]); at += n
    mlist = [gz_member(p, level, False) for p in parts]
    uplain = b"".join(mlist)
    reps = max(1, round(gib * (1 << 30) / UNIT))
    total = reps * UNIT
    plain = torch.frombuffer(bytearray(uplain), dtype=torch.uint8).cuda()
    file = plain.repeat(reps)
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    got = ctypes.c_uint64(0)
    entries = ctypes.c_uint64(0)
    index = torch.empty(2 * (reps * len(parts) + 1), dtype=torch.int64, device="cuda")

    def find():
        rc = zz.lib.zz_members_find_device(ctx._h, file.data_ptr(), file.numel(), 0, index.data_ptr(), index.numel() // 2, ctypes.byref(entries), st)
        assert rc == 0, zz.lib.zz_last_error()

    def check_find():
        assert entries.value == reps * len(parts) + 1 and index[-2:].tolist() == [file.numel(), total]

    def found():
        rc = zz.lib.zz_decode_members_found_device(ctx._h, file.data_ptr(), file.numel(), out.data_ptr(), total, ctypes.byref(got), st)
        assert rc == 0, zz.lib.zz_last_error()

    def check():
        assert got.value == total and bool((out[:total].view(reps, UNIT) == unit).all())
        out.zero_()

    line = {"data": data, "level": level, "layout": layout, "bytes": total, "file_bytes": file.numel(), "members": reps * len(parts)}
    if only != "found":
        ms = timed(find, check_find, min_seconds, stream)
        mid = ms[len(ms) // 2]
        members, cand, dropped, rounds = ctx.last_members_find_stats()
        assert members == reps * len(parts)
        line.update({"candidates": cand, "dropped": dropped, "rounds": rounds, "find_ms": round(mid, 3), "find_ms_min": round(ms[0], 3),
                     "find_ms_max": round(ms[-1], 3), "find_reps": len(ms), "find_gbps": round(total / mid / 1e6, 3)})
    if only != "find":
        ms = timed(found, check, min_seconds, stream)
        mid = ms[len(ms) // 2]
        line.update({"found_ms": round(mid, 3), "found_ms_min": round(ms[0], 3), "found_ms_max": round(ms[-1], 3), "found_reps": len(ms),
                     "found_gbps": round(total / mid / 1e6, 3)})
    if not only:
        # the serial path on the first 16 MiB: one call
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = zz.lib.zz_decode_members_device(ctx._h, plain.data_ptr(), plain.numel(), out.data_ptr(), UNIT, ctypes.byref(got), st)
        e1.record(stream)
        e1.synchronize()
        assert rc == 0 and got.value == UNIT and torch.equal(out[:UNIT], unit) and ctx.last_decode_members_stats()[2] == zz.MEMBERS_SERIAL
        sms = e0.elapsed_time(e1)
        line.update({"serial_ms": round(sms, 1), "serial_mbps": round(UNIT / sms / 1e3, 2),
                     "found_vs_serial": round((total / line["found_ms"]) / (UNIT / sms), 1)})
        out.zero_()
        # the upper bound: the same bytes as a blocked file
        ubc = b"".join(gz_member(host[i:i + CUT], level, True) for i in range(0, UNIT, CUT))
        bfile = torch.frombuffer(bytearray(ubc), dtype=torch.uint8).cuda().repeat(reps)

        def blocked():
            rc = zz.lib.zz_decode_members_device(ctx._h, bfile.data_ptr(), bfile.numel(), out.data_ptr(), total, ctypes.byref(got), st)
            assert rc == 0, zz.lib.zz_last_error()
        ms = timed(blocked, check, min_seconds, stream)
        bmid = ms[len(ms) // 2]
        assert ctx.last_decode_members_stats()[2] == zz.MEMBERS_BLOCKED
        line.update({"blocked_ms": round(bmid, 3), "blocked_gbps": round(total / bmid / 1e6, 3), "found_vs_blocked": round(line["found_ms"] / bmid, 3)})
        # zlib's member loop on one core
        t0 = time.perf_counter()
        n = sum(len(zlib.decompress(m, 31)) for m in mlist)        # (member by member: no copies of the rest of the file)
        zms = 1e3 * (time.perf_counter() - t0)
        assert n == UNIT
        line.update({"zlib_ms": round(zms, 1), "zlib_mbps": round(UNIT / zms / 1e3, 1)})
    print(json.dumps(line), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", action="append", choices=sorted(DATA))
    ap.add_argument("--level", action="append", type=int, choices=list(range(10)))
    ap.add_argument("--layout", action="append", choices=["64k", "loguniform"])
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", choices=["find", "found"])
    a = ap.parse_args()
    for layout in a.layout or ["64k", "loguniform"]:
        for data in a.data or ["text", "mix"]:
            for level in a.level or [1, 6]:
                run(data, level, layout, a.gib, a.min_seconds, a.only)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
