// zz_inflate_members_find.h -- the members of ANY file of gzip members found on the device (zz_members_find_device,
// zz_decode_members_found_device, zz_api.hip): files whose members announce no length -- `cat a.gz b.gz`, append-mode logs, WARC.
// The rules -- zi_mf_candidate, zi_mf_measure, zi_mf_link, zi_mf_again, the slots -- are ZZ_HD functions of zz_inflate_core.h, and
// tests/cxx/members_find_harness.cpp runs the same procedure with them on the host.
//
//   mark    k_members_find_mark<false>  k_members_mark's shape (zz_inflate_members.h), a bandwidth pass: a lane owns 16 offsets and
//                                       tests 1f 8b 08 and the reserved flag bits of every one in registers; only a hit goes back to
//                                       memory for the whole header (zi_mf_candidate). One count per ZZ_MEM_STRETCH bytes.
//           k_members_scan              zz_inflate_members.h's, unchanged: the stretches' bases and the candidate count, which the
//                                       host reads to size every buffer below -- no constant caps the candidates
//           k_members_find_mark<true>   the candidates in ascending order (rank inside the workgroup by a scan over its lanes)
//   reach   k_members_reach             one wavefront per workgroup, persistent, jobs dealt from a counter (k_points_reach's shape,
//                                       sixteen workgroups per CU): job = zi_mf_measure of one candidate. It counts, and writes
//                                       nothing but the candidate's 32-byte record. Round 1: every candidate, all but candidate 0
//                                       with the limit; round 2 (only if the walk met a job that gave up): those the host lists.
//   slots   k_members_find_slots        from the walk's member flags: the members' ranks and the exclusive scan of their `out` (one
//                                       workgroup), k_inflate_items' descriptors of the members in front of m*, m*, the total, and
//                                       the index rows (file offset, decoded offset)
//
// The walk over the records (zi_mf_link) runs on the host, which reads 32 bytes per candidate a round and uploads one flag per
// candidate: a chain is serial by nature, one step per member and no decoding in it. k_inflate_items and k_inflate_members then
// decode, unchanged.
//
// Every kernel reads only [src, src + n) and its workspace and ends for any input: the mark pass reads 20 bytes per lane (byte by
// byte where they would pass the end), zi_header and zi_mf_measure stay inside the bytes they are given.
#pragma once
#include "zz_inflate_members.h"

namespace zz {

#define ZZ_MF_WG_PER_CU 16

// offsets [i, i + 16) are this lane's; a header belongs to the lane that owns its first byte. Bit k: offset i + k is a candidate.
__device__ __forceinline__ uint32_t members_find_mark_lane(const uint8_t* src, uint64_t n, uint64_t i)
{
    if (i >= n) return 0;
    uint32_t d[5] = { 0, 0, 0, 0, 0 };                        // bytes i .. i + 19, zero behind the end
    if (n - i >= 20) {
        uint4 v;
        __builtin_memcpy(&v, src + i, 16);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        d[4] = load32(src + i + 16);
    } else {
        for (uint32_t k = 0; k < (uint32_t)(n - i); ++k) d[k >> 2] |= (uint32_t)src[i + k] << (8 * (k & 3));
    }
    uint32_t hits = 0;                                       // bit k: 1f 8b 08 and a flag byte without reserved bits at i + k
#pragma unroll
    for (uint32_t k = 0; k < ZZ_MEM_PER_LANE; ++k) {
        const uint32_t sh = (k & 3) * 8;
        const uint32_t w = sh ? (d[k >> 2] >> sh) | (d[(k >> 2) + 1] << (32 - sh)) : d[k >> 2];
        hits |= (uint32_t)((w & 0xE0FFFFFFu) == 0x00088B1Fu) << k;
    }
    uint32_t cand = i == 0 ? 1u : 0u;                        // offset 0 is a candidate whatever stands there
    for (uint32_t h = hits; h; h &= h - 1) {                 // rare: the rest of the header comes from memory again
        const uint32_t k = (uint32_t)__builtin_ctz(h);
        if (zi_mf_candidate(src, n, i + k)) cand |= 1u << k;
    }
    return cand;
}

// FILL = false: blk_cnt[b] = candidates in stretch b. FILL = true: the candidates of stretch b from blk_base[b] on, ascending.
template <bool FILL>
__global__ __launch_bounds__(ZZ_MEM_THREADS) void k_members_find_mark(const uint8_t* src, uint64_t n, uint32_t* blk_cnt, const uint64_t* blk_base,
                                                                      uint64_t* offs)
{
    __shared__ uint32_t wtot[ZZ_MEM_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (FILL && blk_cnt[b] == 0) return;                     // uniform: most stretches hold no header
    const uint64_t i = b * ZZ_MEM_STRETCH + (uint64_t)t * ZZ_MEM_PER_LANE;
    const uint32_t cand = members_find_mark_lane(src, n, i);
    const uint32_t mine = (uint32_t)__builtin_popcount(cand);
    const wg_prefix<uint32_t> s = wg_scan_excl<ZZ_MEM_THREADS>(mine, wtot);      // one scan: wtot is not written again
    if (!FILL) { if (t == 0) blk_cnt[b] = s.total; return; }
    uint64_t at = blk_base[b] + s.excl;
    for (uint32_t h = cand; h; h &= h - 1, ++at) offs[at] = i + (uint32_t)__builtin_ctz(h);
}

struct zz_mf_params {
    const uint8_t* src; uint64_t n;
    const uint64_t* offs;                       // the candidates
    zi_find_job* rec;                           // one record per candidate: job k's result goes to rec[k]
    const uint32_t* which;                      // the round's jobs as candidate numbers (nullptr: job i is candidate i)
    uint32_t njobs;
    uint64_t limit;                             // bytes from a job's start (ZI_FIND_NONE: none); candidate 0 never has one
    unsigned int* next;                         // the next job to deal out (zero on entry)
};
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_members_reach(zz_mf_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    zz_inf_lanes w{ (uint8_t*)ibuf4, lane };
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(Q.next, 1u);
        i = uniform(i);
        if (i >= Q.njobs) break;
        const uint32_t k = Q.which ? Q.which[i] : i;
        const zi_find_job j{ Q.offs[k], 0, zi_mf_limit(k, Q.limit), 0, 0 };
        const zi_find_job r = zi_mf_measure(w, Q.src, Q.n, j, S, lane, ZZ_INF_THREADS);
        if (lane == 0) Q.rec[k] = r;
        __syncthreads();                        // the next job's first stage overwrites the input buffer
    }
}

// what the host reads behind the slots (zeroed, mstar ~0, in front of the launch)
struct zz_mf_state {
    unsigned long long members;      // members of the walk
    unsigned long long total;        // sum of their `out`
    unsigned long long mstar;        // first member that passes cap (~0: none),
    unsigned long long mstar_src;    //   where it begins in the source
    unsigned long long mstar_dst;    //   and in the destination
};
struct zz_mf_slots {
    const uint8_t* src; uint64_t n; uint8_t* dst; uint64_t cap;
    const zi_find_job* rec; const uint8_t* keep; uint64_t nc;                       // the candidates' records, the walk's flags
    const uint8_t** srcs; uint64_t* src_lens; uint8_t** dsts; uint64_t* caps;      // k_inflate_items' descriptors (srcs == nullptr: none)
    uint64_t* idx;                                                                  // members + 1 index rows (nullptr: none)
    zz_mf_state* st;
};
// one workgroup, 1024 candidates a round: the members' ranks and the exclusive scan of their `out` between one pair of barriers
__global__ __launch_bounds__(ZZ_MEM_SCAN_THREADS) void k_members_find_slots(zz_mf_slots Q)
{
    __shared__ uint32_t wrank[ZZ_MEM_SCAN_THREADS / ZZ_WAVE];
    __shared__ uint64_t woff[ZZ_MEM_SCAN_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    uint32_t members = 0;                                    // (at most 2^31 - 1 candidates)
    uint64_t total = 0;
    for (uint64_t r0 = 0; r0 < Q.nc; r0 += ZZ_MEM_SCAN_THREADS) {
        const uint64_t k = r0 + t;
        const bool kept = k < Q.nc && Q.keep[k] != 0;
        uint64_t c = 0, used = 0, out = 0;
        if (kept) { const zi_find_job r = Q.rec[k]; c = r.a; used = r.b; out = r.c; }
        const wg_prefix2<uint32_t, uint64_t> s = wg_scan_excl2<ZZ_MEM_SCAN_THREADS>(kept ? 1u : 0u, wrank, out, woff, members, total);
        if (kept) {
            const uint64_t j = s.a.excl, off = s.b.excl;
            if (Q.idx) { Q.idx[2 * j] = c; Q.idx[2 * j + 1] = off; }
            if (Q.srcs && zi_mf_dealt(out, off, Q.cap)) {
                Q.srcs[j] = Q.src + c; Q.src_lens[j] = used;
                Q.dsts[j] = Q.dst + off; Q.caps[j] = out;
            }
            if (zi_mf_is_mstar(out, off, Q.cap)) { Q.st->mstar = j; Q.st->mstar_src = c; Q.st->mstar_dst = off; }   // (one member at most)
        }
        members += s.a.total; total += s.b.total;
        __syncthreads();
    }
    if (t == 0) {
        Q.st->members = members; Q.st->total = total;
        if (Q.idx) { Q.idx[2 * (uint64_t)members] = Q.n; Q.idx[2 * (uint64_t)members + 1] = total; }
    }
}

}  // namespace zz
