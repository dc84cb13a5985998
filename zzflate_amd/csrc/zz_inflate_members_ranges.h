// zz_inflate_members_ranges.h -- many reads of one blocked gzip (BGZF) file through its index in one call
// (zz_decode_members_ranges_device, zz_api.hip), and the index made on the device from the file alone (zz_members_index_device).
// The rules -- what an index is, which members a read touches, ranks, rooms, waves, the cut and the verdict -- are ZZ_HD functions
// of zz_inflate_core.h (zi_mr_*); tests/cxx/inflate_members_ranges_harness.cpp runs the same procedure with them on the host.
//
//   check    k_mr_check     one thread per entry, one flag: is the index an index?
//   plan     k_mr_plan      one thread per read: status, m, first and last touched member (two binary searches over the decoded
//                           offsets), +1 / -1 in the difference array over the members. A bad index settles every read here.
//   touched  k_mr_touched   one workgroup, 1024 members a round: coverage from the differences, the touched flags, their count
//                           in front of every member, the touched list, S (exclusive sum of rooms) and G (big members)
//            k_mr_waves     one thread per wave: its first rank and S there -- what the host sizes stage and launches by
//   per wave k_mr_desc      one thread per rank: k_inflate_items' descriptor (src + c_j, c_(j+1) - c_j, stage + S_j - S_wave, room)
//            k_inflate_items   unchanged (zz_inflate.h), with a status array
//            k_mr_judge     one workgroup: F over the wave's ranks, carried on from the wave in front of it
//            k_mr_cut       one workgroup: per read the chunks of its interval in this wave (zi_mr_cut), their exclusive scan
//            k_mr_copy      a fixed grid deals the chunks out: the read by binary search over the scan, ZZ_MR_CHUNK bytes by
//                           coop_copy (16-byte stores aligned on the destination); a long read is many workgroups' work
//   verdict  k_mr_verdict   one thread per read: d_out_lens, d_status and the four counters the host reads
//
// The host reads zz_mr_state once, two words per wave once, and k_inflate_items' two counters per wave, whatever the numbers of
// reads and members are.
//
// Workspace: the stage (the largest wave's rooms: below 2 * ZZ_MR_STAGE = 128 MiB), 28 bytes per member (differences, counts,
// touched list, S, F, G), 44 bytes per touched member of the largest wave (k_inflate_items' descriptors, lengths and statuses),
// 32 bytes per read (its record and the chunk scan), 16 bytes per wave.
//
// Bounds, for any index and any read array: nothing runs past k_mr_plan unless the index passed the check, so c_(j+1) <= src_len
// and rooms are differences of an ascending sequence; a descriptor gives zi_item exactly src[c_j, c_(j+1)) and a slot of `room`
// bytes inside the stage, which holds the wave's sum of rooms; a piece lies inside the slots of its read's members and
// dst_off + len <= m <= cap (zi_mr_cut), and reads with m > cap are copied nowhere.
#pragma once
#include "zz_inflate_members.h"

namespace zz {

#define ZZ_MR_SCAN_THREADS 1024
#define ZZ_MR_COPY_GRID 2048

// what the host reads (all of it written by the device)
struct zz_mr_state {
    unsigned long long index_bad;      // k_mr_check (zeroed in front of a call)
    unsigned long long touched;        // k_mr_touched: touched members, the big ones among them, the sum of rooms, waves
    unsigned long long big;
    unsigned long long stage_total;
    unsigned long long nwaves;
    unsigned long long n_data, n_unsupported, n_arg, n_nospace;      // k_mr_plan / k_mr_verdict: reads with these (zeroed)
};

struct zz_mr_params {
    const uint8_t* src; uint64_t src_len;
    const uint64_t* idx; uint64_t entries;
    uint64_t nranges; const uint64_t* firsts; const uint64_t* nbytes; uint8_t* const* dsts; const uint64_t* caps;
    uint64_t* out_lens; int32_t* status;            // status may be null
    zi_mr_read* reads; uint64_t* chunk0;            // per read: its record; first chunk of the wave being copied (nranges + 1)
    int32_t* diff; uint32_t* cnt;                   // per member (+ 1)
    uint32_t* tlist; uint64_t* S; uint32_t* F; uint32_t* G;      // per touched member (+ 1)
    uint8_t* stage;
    zz_mr_state* st;
};
__device__ __forceinline__ zi_mr_tables mr_tables(const zz_mr_params& Q)
{
    const uint64_t T = Q.st->touched;
    return zi_mr_tables{ { Q.idx, 2 * Q.entries }, { Q.cnt, Q.entries }, { Q.tlist, T }, { Q.S, T + 1 }, { Q.F, T + 1 }, { Q.G, T + 1 } };
}

// one pass, one flag (every writer stores the same value)
__global__ __launch_bounds__(256) void k_mr_check(zz_mr_params Q)
{
    const zi_view<const uint64_t> idx{ Q.idx, 2 * Q.entries };
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < Q.entries; j += stride)
        if (zi_mr_entry_bad(idx, Q.entries, j, Q.src_len)) Q.st->index_bad = 1ull;
}

__global__ __launch_bounds__(256) void k_mr_plan(zz_mr_params Q)
{
    const zi_view<const uint64_t> idx{ Q.idx, 2 * Q.entries };
    const bool bad = Q.st->index_bad != 0;                  // uniform
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < Q.nranges; r += stride) {
        if (bad) {                                          // not an index: the call fails as a whole
            Q.out_lens[r] = ~0ull;
            if (Q.status) Q.status[r] = ZI_RV_DATA;
            continue;
        }
        const zi_mr_read R = zi_mr_plan(idx, Q.entries, Q.firsts[r], Q.nbytes[r], Q.caps[r]);
        Q.reads[r] = R;
        if (R.any) { atomicAdd(&Q.diff[R.j0], 1); atomicSub(&Q.diff[(uint64_t)R.j1 + 1], 1); }
    }
}

// One workgroup, 1024 members a round, three scans a round. Coverage is summed in 32 bits: every prefix of the differences from
// member 0 on lies in [0, nranges], nranges < 2^31, so the wrapped sum is the true one. The touched and the big members of a
// round are counted in one word (16 bits each: a round holds 1024).
__global__ __launch_bounds__(ZZ_MR_SCAN_THREADS) void k_mr_touched(zz_mr_params Q)
{
    __shared__ uint32_t wcov[ZZ_MR_SCAN_THREADS / ZZ_WAVE], wcnt[ZZ_MR_SCAN_THREADS / ZZ_WAVE];
    __shared__ uint64_t wroom[ZZ_MR_SCAN_THREADS / ZZ_WAVE];
    const zi_view<const uint64_t> idx{ Q.idx, 2 * Q.entries };
    const uint64_t members = Q.entries - 1;
    const uint32_t t = threadIdx.x;
    if (Q.st->index_bad) return;                             // uniform: k_mr_plan settled every read
    uint32_t ccov = 0; uint64_t ccnt = 0, cbig = 0, croom = 0;
    for (uint64_t r0 = 0; r0 < members; r0 += ZZ_MR_SCAN_THREADS) {
        const uint64_t j = r0 + t;
        const uint32_t d = j < members ? (uint32_t)Q.diff[j] : 0u;
        const wg_prefix<uint32_t> sc = wg_scan_excl<ZZ_MR_SCAN_THREADS>(d, wcov, ccov);
        const uint32_t cov = sc.excl + d;                      // the reads that cover member j (inclusive; wraps to the true sum)
        const uint64_t room = j < members ? zi_mr_room(idx, j) : 0;
        const uint32_t kind = j < members ? zi_mr_touch(room, (int32_t)cov) : 0u;
        const uint32_t one = (kind ? 1u : 0u) | (kind == 2 ? 0x10000u : 0u);
        const uint64_t myroom = kind == 1 ? room : 0;
        const wg_prefix2<uint32_t, uint64_t> s = wg_scan_excl2<ZZ_MR_SCAN_THREADS>(one, wcnt, myroom, wroom, 0u, croom);
        const uint64_t bcnt = ccnt + (s.a.excl & 0xFFFFu), bbig = cbig + (s.a.excl >> 16), broom = s.b.excl;
        if (j < members) {
            Q.cnt[j] = (uint32_t)bcnt;
            if (kind) {
                Q.tlist[bcnt] = (uint32_t)j | (kind == 2 ? ZI_MR_BIG : 0u);
                Q.S[bcnt] = broom; Q.G[bcnt] = (uint32_t)bbig;
            }
        }
        ccov += sc.total; ccnt += s.a.total & 0xFFFFu; cbig += s.a.total >> 16; croom += s.b.total;
        __syncthreads();                                     // (and what this round wrote is the workgroup's to read)
    }
    if (t == 0) {
        Q.cnt[members] = (uint32_t)ccnt;
        Q.S[ccnt] = croom; Q.G[ccnt] = (uint32_t)cbig; Q.F[0] = 0;
        Q.st->touched = ccnt; Q.st->big = cbig; Q.st->stage_total = croom;
        Q.st->nwaves = ccnt ? zi_mr_wave(Q.S[ccnt - 1]) + 1 : 0;                 // the last touched member's wave is the last
    }
}

// wave w begins at rank tab[2w] with S = tab[2w + 1]; entry `nwaves` is (T, the sum of rooms)
__global__ __launch_bounds__(256) void k_mr_waves(zz_mr_params Q, uint64_t nwaves, uint64_t* tab)
{
    const uint64_t T = Q.st->touched;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= nwaves; w += stride) {
        const uint64_t t = w < nwaves ? zi_mr_wave_first(zi_view<const uint64_t>{ Q.S, T + 1 }, T, w * ZZ_MR_STAGE) : T;
        tab[2 * w] = t; tab[2 * w + 1] = Q.S[t];
    }
}

// ranks [t0, t1) are the wave's: k_inflate_items' descriptors
__global__ __launch_bounds__(256) void k_mr_desc(zz_mr_params Q, uint64_t t0, uint64_t t1, const uint8_t** srcs, uint64_t* src_lens,
                                                 uint8_t** dsts, uint64_t* caps)
{
    const zi_mr_tables T = mr_tables(Q);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t0 + i < t1; i += stride) {
        const zi_mr_slot s = zi_mr_desc(T, t0 + i, t0, Q.src_len);
        srcs[i] = Q.src + s.src_off; src_lens[i] = s.src_len; dsts[i] = Q.stage + s.stage_off; caps[i] = s.room;
    }
}

// one workgroup: F[t + 1] for the ranks of the wave, from what k_inflate_items said about each (item i is rank t0 + i)
__global__ __launch_bounds__(ZZ_MR_SCAN_THREADS) void k_mr_judge(zz_mr_params Q, uint64_t t0, uint64_t t1, const uint64_t* caps,
                                                                 const uint64_t* out_lens, const int32_t* status)
{
    __shared__ uint32_t wtot[ZZ_MR_SCAN_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    uint32_t carry = Q.F[t0];
    for (uint64_t r0 = t0; r0 < t1; r0 += ZZ_MR_SCAN_THREADS) {
        const uint64_t k = r0 + t;
        const uint32_t bad = k < t1 && zi_mr_member_bad(Q.tlist[k], status[k - t0], out_lens[k - t0], caps[k - t0]) ? 1u : 0u;
        const wg_prefix<uint32_t> s = wg_scan_excl<ZZ_MR_SCAN_THREADS>(bad, wtot, carry);
        if (k < t1) Q.F[k + 1] = s.excl + bad;           // inclusive: the bad members up to and with rank k
        carry += s.total;
        __syncthreads();
    }
}

// one workgroup: chunk0[r] = the chunks of the reads in front of r in this wave, chunk0[nranges] = all of them
__global__ __launch_bounds__(ZZ_MR_SCAN_THREADS) void k_mr_cut(zz_mr_params Q, uint64_t t0, uint64_t t1)
{
    __shared__ uint64_t wtot[ZZ_MR_SCAN_THREADS / ZZ_WAVE];
    const zi_mr_tables T = mr_tables(Q);
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t r0 = 0; r0 < Q.nranges; r0 += ZZ_MR_SCAN_THREADS) {
        const uint64_t r = r0 + t;
        const uint64_t mine = r < Q.nranges ? zi_mr_chunks(zi_mr_cut(Q.reads[r], Q.firsts[r], T, t0, t1).len) : 0;
        const wg_prefix<uint64_t> s = wg_scan_excl<ZZ_MR_SCAN_THREADS>(mine, wtot, carry);
        if (r < Q.nranges) Q.chunk0[r] = s.excl;
        carry += s.total;
        __syncthreads();
    }
    if (t == 0) Q.chunk0[Q.nranges] = carry;
}

// chunk g belongs to the read r with chunk0[r] <= g < chunk0[r + 1]; it is bytes [k * ZZ_MR_CHUNK, ..) of the read's piece
__global__ __launch_bounds__(256) void k_mr_copy(zz_mr_params Q, uint64_t t0, uint64_t t1)
{
    const zi_mr_tables T = mr_tables(Q);
    const uint64_t all = Q.chunk0[Q.nranges];
    for (uint64_t g = blockIdx.x; g < all; g += gridDim.x) {
        uint64_t lo = 0, hi = Q.nranges;                     // chunk0[lo] <= g < chunk0[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (Q.chunk0[mid] <= g) lo = mid;
            else hi = mid;
        }
        const zi_mr_piece p = zi_mr_cut(Q.reads[lo], Q.firsts[lo], T, t0, t1);
        const uint64_t at = (g - Q.chunk0[lo]) * ZZ_MR_CHUNK;
        if (at >= p.len) continue;                           // (cannot happen: the read owns this chunk)
        // the chunk is the workgroup's, so its three numbers are scalars: the copy keeps its registers for the bytes in flight
        const uint64_t n = uniform64(p.len - at < ZZ_MR_CHUNK ? p.len - at : ZZ_MR_CHUNK);
        uint8_t* const d = (uint8_t*)uniform64((uint64_t)(uintptr_t)(Q.dsts[lo] + p.dst_off + at));
        const uint8_t* const s = (const uint8_t*)uniform64((uint64_t)(uintptr_t)(Q.stage + p.stage_off + at));
        coop_copy(d, s, n, threadIdx.x, blockDim.x);
    }
}

__global__ __launch_bounds__(256) void k_mr_verdict(zz_mr_params Q)
{
    const zi_mr_tables T = mr_tables(Q);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < Q.nranges; r += stride) {
        const zi_mr_read R = Q.reads[r];
        const int v = zi_mr_verdict(R, T);
        Q.out_lens[r] = v == ZI_RV_OK ? R.m : ~0ull;
        if (Q.status) Q.status[r] = v;
        if (v == ZI_RV_DATA) atomicAdd(&Q.st->n_data, 1ull);
        else if (v == ZI_RV_UNSUPPORTED) atomicAdd(&Q.st->n_unsupported, 1ull);
        else if (v == ZI_RV_ARG) atomicAdd(&Q.st->n_arg, 1ull);
        else if (v == ZI_RV_NOSPACE) atomicAdd(&Q.st->n_nospace, 1ull);
    }
}

// ---- the index from the file alone (zz_members_index_device): behind mark, scan, fill, check and hop of zz_inflate_members.h ----
// one workgroup, 1024 members a round: (c_j, exclusive sum of ISIZE) per member, and the last pair (the end of the last member, the sum)
__global__ __launch_bounds__(ZZ_MR_SCAN_THREADS) void k_members_pairs(const uint8_t* src, uint64_t n, const uint64_t* offs, const uint32_t* lens,
                                                                      uint64_t m, uint64_t* idx)
{
    __shared__ uint64_t wtot[ZZ_MR_SCAN_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t r0 = 0; r0 < m; r0 += ZZ_MR_SCAN_THREADS) {
        const uint64_t j = r0 + t;
        uint64_t c = 0; uint32_t len = 0, isize = 0;
        if (j < m) { c = offs[j]; len = lens[j]; isize = zi_members_isize(zi_view<const uint8_t>{ src, n }, c, len); }
        const wg_prefix<uint64_t> s = wg_scan_excl<ZZ_MR_SCAN_THREADS>((uint64_t)isize, wtot, carry);
        const uint64_t off = s.excl;
        if (j < m) {
            idx[2 * j] = c; idx[2 * j + 1] = off;
            if (j + 1 == m) { idx[2 * m] = c + len; idx[2 * m + 1] = off + isize; }
        }
        carry += s.total;
        __syncthreads();
    }
}

}  // namespace zz
