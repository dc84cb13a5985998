"""Indexed reads of a blocked (BGZF) gzip file on one GPU (zz_decode_members_ranges_device): one JSON line per row.

    python tools/bench_decode_members_ranges.py [--level 1|6 ...] [--gib 1] [--min-seconds 0.5] [--reads N ...] [--only reads] [--out FILE]

The file is tools/bench_decode_members.py's: about --gib GiB of decoded text as blocked members of 65,280 input bytes each, a
16 MiB unit (zz_generate_device) that host zlib compresses member by member, repeated. Per level:
  index         one row: the median zz_members_index_device call over the file (the index is made once and timed by itself)
  members       one row: the median zz_decode_members_device call over the whole file -- what a caller without this call pays
                to serve any read
  reads         one row per count (1, 64, 768, 4,096 and 65,536 by default): the median call with that many seeded 4 KiB reads at
                random offsets; `vs_members` is its time over the `members` row's, measured in this process
  one 64 MiB    one row each: a call with a single read of 64 MiB, and one with a single read of the whole file
  / whole read
Times are HIP events on the launch stream around a call (the calls are synchronous), after a warm-up, repeated until
--min-seconds of timed work; the destinations are compared with the input on the device after the warm-up and after the last
timed call, outside the clock. The 768-read row is held to its requirement: at most half the `members` row's time.
--only reads runs nothing but the timed read calls (for a kernel trace of its own).
"""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import zzflate_amd as zz  # noqa: E402
from bench_decode_members import gz_member, UNIT, CUT  # noqa: E402

READ = 4096


def timed(fn, check, min_seconds, stream):
    """ms of fn() between HIP events (sorted): warm-up and check first, then calls until min_seconds of timed work, then check"""
    fn()
    torch.cuda.synchronize()
    check()
    ms = []
    while sum(ms) < 1e3 * min_seconds or len(ms) < 5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    check()
    ms.sort()
    return ms


def summary(ms):
    return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "reps": len(ms)}


def run(level, gib, min_seconds, counts, only, emit):
    ctx = zz.Context(0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    unit = torch.empty(UNIT, dtype=torch.uint8, device="cuda")
    ctx.generate(zz.GEN_TEXT, 1, 0, unit, UNIT)
    host = unit.cpu().numpy().tobytes()
    parts = [host[i:i + CUT] for i in range(0, UNIT, CUT)]
    reps = max(1, round(gib * (1 << 30) / UNIT))
    total = reps * UNIT
    file = torch.frombuffer(bytearray(b"".join(gz_member(p, level, True) for p in parts)), dtype=torch.uint8).cuda().repeat(reps)
    out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    base = {"data": "text", "level": level, "bytes": total, "file_bytes": file.numel(), "members": reps * len(parts)}

    # the index, made once and timed by itself
    entries = ctypes.c_uint64(0)
    index = torch.empty((base["members"] + 1, 2), dtype=torch.int64, device="cuda")

    def make_index():
        rc = zz.lib.zz_members_index_device(ctx._h, file.data_ptr(), file.numel(), index.data_ptr(), index.shape[0], ctypes.byref(entries), st)
        assert rc == 0, zz.lib.zz_last_error()

    def check_index():
        assert entries.value == index.shape[0] and int(index[-1, 0]) == file.numel() and int(index[-1, 1]) == total

    ms = timed(make_index, check_index, min_seconds, stream)
    if not only:
        emit({**base, "row": "index", **summary(ms)})

    # the whole file through zz_decode_members_device, beside the reads
    members_ms = None
    if not only:
        got = ctypes.c_uint64(0)

        def members():
            rc = zz.lib.zz_decode_members_device(ctx._h, file.data_ptr(), file.numel(), out.data_ptr(), total, ctypes.byref(got), st)
            assert rc == 0, zz.lib.zz_last_error()

        def check_members():
            assert got.value == total and bool((out[:total].view(reps, UNIT) == unit).all())
            out.zero_()

        ms = timed(members, check_members, min_seconds, stream)
        members_ms = ms[len(ms) // 2]
        emit({**base, "row": "members", **summary(ms), "gbps": round(total / members_ms / 1e6, 3)})

    def reads_row(name, firsts, nbytes):
        """one call's row: the reads' destinations follow one another in `out`"""
        k = len(firsts)
        offs = [0]
        for n in nbytes:
            offs.append(offs[-1] + n)
        assert offs[-1] <= total
        tab = torch.tensor([firsts, nbytes, [out.data_ptr() + o for o in offs[:-1]], nbytes], dtype=torch.int64).cuda()
        lens = torch.zeros(k, dtype=torch.int64, device="cuda")
        status = torch.zeros(k, dtype=torch.int32, device="cuda")

        def call():
            rc = zz.lib.zz_decode_members_ranges_device(ctx._h, file.data_ptr(), file.numel(), index.data_ptr(), index.shape[0], k, tab[0].data_ptr(),
                                                        tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), lens.data_ptr(), status.data_ptr(), st)
            assert rc == 0, zz.lib.zz_last_error()

        def check():
            assert bool((status == 0).all()) and torch.equal(lens, tab[1])
            if max(nbytes) == READ:                               # small reads: the decoded file is the unit repeated, so a gather
                lane = torch.arange(READ, device="cuda")[None, :]
                for r0 in range(0, k, 2048):
                    want = unit[(tab[0][r0:r0 + 2048, None] + lane) % UNIT]
                    assert torch.equal(out[offs[r0]:offs[r0] + want.numel()].view(-1, READ), want), (name, r0)
            else:                                                 # a long read: the rest of a unit, whole units, the head of one
                for a, n, o in zip(firsts, nbytes, offs):
                    got = out[o:o + n]
                    head = min(n, (-a) % UNIT)
                    body = (n - head) // UNIT
                    tail = n - head - body * UNIT
                    assert torch.equal(got[:head], unit[a % UNIT:a % UNIT + head]), name
                    assert bool((got[head:head + body * UNIT].view(body, UNIT) == unit).all()), name
                    assert torch.equal(got[n - tail:], unit[:tail]), name
            out[:offs[-1]].zero_()

        ms = timed(call, check, min_seconds, stream)
        dec, waves = ctx.last_decode_members_ranges_stats()
        row = {**base, "row": name, "reads": k, "read_bytes": offs[-1], **summary(ms), "members_decoded": dec, "waves": waves}
        if members_ms is not None:
            row["vs_members"] = round(row["ms"] / members_ms, 3)
        emit(row)
        return row

    rng = random.Random(12)
    for k in counts:
        row = reads_row("reads", [rng.randrange(total - READ) for _ in range(k)], [READ] * k)
        if k == 768 and members_ms is not None:
            assert row["ms"] <= 0.5 * members_ms, f"768 reads take {row['ms']} ms, the whole file {members_ms} ms: more than half"
    if not only:
        reads_row("one 64 MiB read", [rng.randrange(total - (64 << 20))], [64 << 20])
        reads_row("one whole-file read", [0], [total])
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", action="append", type=int, choices=list(range(10)))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--reads", action="append", type=int)
    ap.add_argument("--only", choices=["reads"])
    ap.add_argument("--out", help="append every row to this file too")
    a = ap.parse_args()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    for level in a.level or [1, 6]:
        run(level, a.gib, a.min_seconds, a.reads or [1, 64, 768, 4096, 65536], a.only, emit)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
