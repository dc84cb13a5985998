// zz_inflate_points_ranges.h -- many reads of ANY zlib / gzip / raw stream through a point index with windows in one call
// (zz_decode_points_ranges_device, zz_api.hip). The rules -- the sidecar, zi_out_window, the fold (zi_pr_*) -- are ZZ_HD functions
// of zz_inflate_core.h; tests/cxx/inflate_points_ranges_harness.cpp runs the same procedure with them on the host.
//
// A point index has the shape of a member index, so everything that looks only at the decoded offsets is zz_inflate_members_ranges.h
// called with the rows: k_mr_check (the last bit bounded by eight times the source), k_mr_plan, k_mr_touched, k_mr_waves, k_mr_judge,
// k_mr_cut, k_mr_copy, k_mr_verdict. New here:
//
//   front    k_pr_front               one workgroup: the container header, row 0's bit, the last row's bit against the trailer's place, and
//                                     the fold of the sums over the index's 64-bit lengths against the trailer -- every thread joins a
//                                     run of consecutive entries, a tree joins the runs in order. What it refuses is "not an
//                                     index" to k_mr_plan: every read fails, nothing else is launched.
//   per wave k_inflate_segments_win   k_inflate_segments' shape: one wavefront per workgroup, persistent, the wave's ranks dealt
//                                     from a counter. The wavefront reads its rank's rows, decodes the segment onto its slot of the
//                                     stage (zi_out_window: plain stores; a source in front of the segment is read from the window
//                                     slot in d_windows where it lies -- the LDS holds the tables and the 2 KiB input stage, nothing
//                                     else), sums the slot (zi_adler_lanes / zi_crc_lanes, as zi_item does) and writes the verdict in
//                                     k_inflate_items' words, so that k_mr_judge counts F from it. No bitmap, no pointers: nothing is
//                                     pending.
//
// Workspace beside zz_inflate_members_ranges.h's per read, per segment and per wave: the stage, 20 bytes per touched segment of the
// largest wave (room, bytes, status) and this file's state. The fold needs none: it reads the sums where they are.
//
// Bounds, for any index, sidecar and read array: nothing runs past k_mr_plan unless k_mr_check and k_pr_front accepted, so the bits
// ascend up to at most 8 * sn and the rooms are differences of an ascending sequence; a segment's run reads only the DEFLATE bytes
// s[0, sn) (zz_inf_in), its window slot d_windows[seg * 32768, + 32768) -- at a distance the stream itself allows -- and writes only
// its slot of `room` bytes inside the stage, which holds the wave's sum of rooms.
#pragma once
#include "zz_inflate_points.h"
#include "zz_inflate_members_ranges.h"

namespace zz {

#define ZZ_PR_FRONT_THREADS 1024

// what k_pr_front leaves for the kernels behind it and for the host
struct zz_pr_state {
    unsigned long long hl, sn;         // the container header's length, the DEFLATE bytes
    unsigned long long dict;           // the header asks for a preset dictionary
    unsigned long long refused;        // header, last bit, an entry or the fold: the call fails as a whole
    unsigned int next, pad;            // the next rank of the wave to deal out (zero on entry)
};
struct zz_pr_params {
    const uint8_t* src; uint64_t src_len; int format;
    const uint8_t* windows; const uint32_t* sums;
    zz_pr_state* ps;
    uint64_t* rooms; uint64_t* out_lens; int32_t* status;      // per rank of a wave: what k_mr_judge reads
};

__global__ __launch_bounds__(ZZ_PR_FRONT_THREADS) void k_pr_front(zz_mr_params Q, zz_pr_params P)
{
    __shared__ uint32_t pv[ZZ_PR_FRONT_THREADS];
    __shared__ uint64_t pl[ZZ_PR_FRONT_THREADS];
    __shared__ uint32_t entry_bad;
    const zi_view<const uint64_t> idx{ Q.idx, 2 * Q.entries };
    const uint64_t segments = Q.entries - 1;
    const int kind = zi_sidecar_kind(P.format);
    const uint32_t t = threadIdx.x;
    if (t == 0) entry_bad = 0;
    __syncthreads();
    // thread t joins the entries [t * per, (t + 1) * per); lengths wrap where the rows do not ascend, and then k_mr_check has refused
    const uint64_t per = (segments + ZZ_PR_FRONT_THREADS - 1) / ZZ_PR_FRONT_THREADS;
    const uint64_t j0 = (uint64_t)t * per < segments ? (uint64_t)t * per : segments, j1 = j0 + per < segments ? j0 + per : segments;
    zi_pr_part acc{ 0, 0 };
    bool bad = false;
    for (uint64_t j = j0; j < j1; ++j) {
        zi_pr_part p;
        if (!zi_pr_entry_part(kind, P.sums[j], zi_mr_u(idx, j + 1) - zi_mr_u(idx, j), &p)) bad = true;
        acc = zi_pr_join(kind, acc, p);
    }
    if (bad) atomicOr(&entry_bad, 1u);
    pv[t] = acc.v; pl[t] = acc.len;
    __syncthreads();
    for (uint32_t s = 1; s < ZZ_PR_FRONT_THREADS; s <<= 1) {
        if ((t & (2 * s - 1)) == 0) {
            const zi_pr_part x = zi_pr_join(kind, zi_pr_part{ pv[t], pl[t] }, zi_pr_part{ pv[t + s], pl[t + s] });
            pv[t] = x.v; pl[t] = x.len;
        }
        __syncthreads();
    }
    if (t != 0) return;
    const int64_t hl = zi_header(P.format, P.src, P.src_len);
    uint64_t sn = 0;
    const uint64_t tl = P.format == 0 ? 4 : P.format == 1 ? 8 : 0;
    const bool ok = zi_pr_deflate_len(P.format, P.src_len, hl, &sn) && zi_pr_ends_ok(zi_mr_c(idx, 0), zi_mr_c(idx, segments), sn) && !entry_bad &&
                    zi_pr_trailer_ok(P.format, P.src + (P.src_len - tl), zi_pr_part{ pv[0], zi_mr_u(idx, segments) });
    P.ps->hl = hl < 0 ? 0ull : (unsigned long long)hl; P.ps->sn = sn;
    P.ps->dict = hl == -2 ? 1ull : 0ull;
    P.ps->refused = ok ? 0ull : 1ull;
    if (!ok) Q.st->index_bad = 1ull;
}

// ranks [t0, t1) are the wave's; rank t0 + i writes rooms[i], out_lens[i], status[i]
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_segments_win(zz_mr_params Q, zz_pr_params P, uint64_t t0, uint64_t t1)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    const zi_mr_tables T = mr_tables(Q);
    const uint8_t* const s = P.src + P.ps->hl;
    const uint64_t sn = P.ps->sn;
    const int kind = zi_sidecar_kind(P.format);
    zz_inf_lanes w{ (uint8_t*)ibuf4, lane };
    for (;;) {
        // lane 0 draws the rank, every lane gets its number
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(&P.ps->next, 1u);
        i = uniform(i);
        if (i >= t1 - t0) break;
        const zi_pr_slot d = zi_pr_desc(T, Q.entries, t0 + i, t0);
        int status = ZI_ITEM_DATA;
        uint64_t out = ~0ull;
        if (!d.skip) {
            S.kind = 0;
            const zi_view<const uint8_t> view{ s, sn };
            zz_inf_in in{ s, sn, (uint8_t*)ibuf4, -(int64_t)(2 * ZZ_INF_IBUF), lane };
            zi_out_window<zz_inf_fence> o{ zi_view<uint8_t>{ Q.stage + d.stage_off, d.room },
                                           zi_view<const uint8_t>{ P.windows + d.seg * ZI_PR_WINDOW, ZI_PR_WINDOW }, d.o0, 0, 0, lane,
                                           ZZ_INF_THREADS, {} };
            zi_pt_segment pt{ (uint32_t)(d.b0 & 7), d.b1, d.last, 0 };
            const zi_result R = zi_run(in, view, d.b0 >> 3, o, S, ZI_RUN_POINT, d.room, lane, ZZ_INF_THREADS, pt);
            uint32_t sum = 0;
            if (!R.err) {                                   // the run produced exactly the room: sum the slot
                w.sync();
                const zi_view<const uint8_t> slot{ Q.stage + d.stage_off, d.room };
                sum = kind == ZI_CKS_ADLER ? zi_adler_lanes(w, slot, d.room, lane, ZZ_INF_THREADS) : zi_crc_lanes(w, slot, d.room, lane, ZZ_INF_THREADS);
            }
            status = zi_pr_segment_status(R.err, R.out, d.room, sum, P.sums[d.seg]);
            if (status == ZI_ITEM_OK) out = R.out;
        }
        if (lane == 0) { P.rooms[i] = d.room; P.out_lens[i] = out; P.status[i] = status; }
        __syncthreads();                        // the next segment's first stage overwrites the input buffer
    }
}

}  // namespace zz
