// zz_inflate_points.h -- decode of ANY zlib / gzip / raw stream in parallel from a point index (zz_decode_points_device, zz_api.hip;
// the rules -- ZI_RUN_POINT, zi_out_segment, zi_points_check, zi_points_batches, the builder -- are in zz_inflate_core.h, and
// tests/cxx/inflate_points_harness.cpp runs them on the CPU).
//
//   phase 1  k_inflate_segments   one wavefront per workgroup, persistent, the batch's segments dealt from a counter (the shape
//                                 of k_inflate_items). A segment is the blocks between two rows of the index: the wavefront reads
//                                 its two rows, stages input from the byte that holds in_bit and decodes straight onto the
//                                 destination -- the window IS the destination, so the LDS holds the tables and the 2 KiB input
//                                 stage and nothing else (9,232 bytes: sixteen workgroups on a CU). A byte whose source lies in
//                                 front of the segment is PENDING: its bit in the batch's bitmap (global memory, atomicOr: two
//                                 segments may share a word) and its pointer in st.
//   count    k_points_count       segments and tiles do not line up, so phase 1 keeps no per-tile counts: one pass over the
//                                 bitmap pop-counts every tile of ZI_POINTS_TILE bytes into pcnt / prem and the total into tot[ZZ_TOT_PENDING].
//   phase 2  k_inflate_resolve    zz_inflate.h's rounds, unchanged: they never looked at packets, only at tiles of P bytes
//                                 through pend, st, pcnt and prem.
//
// Every kernel reads only the DEFLATE bytes s[0, sn) and its workspace, and writes only its segment's bytes of the destination
// (zi_out_segment's capacity is the segment's announced length) and the workspace of its batch; the host has checked the rows
// (zi_points_check) before any of them is launched.
#pragma once
#include "zz_inflate.h"

namespace zz {

#define ZZ_PT_BATCH_SEGMENTS (1u << 20)         // segments per batch at the most (rows and results: 32 bytes each)
#define ZZ_PT_WG_PER_CU 16                      // resident workgroups (= wavefronts) per CU the grid is sized for

// a segment's result
struct zz_pt_stat {
    uint64_t end_bit;                           // where its run ended
    uint32_t flags;                             // bit 0 ok, bit 1 it ended with the final block
    uint32_t bytes;                             // bytes it produced
};
struct zz_pt_params {
    const uint8_t* s; uint64_t sn;              // the DEFLATE bytes (no trailer)
    const uint64_t* rows;                       // the batch's rows: nseg + 1 of them
    uint32_t nseg; int last;                    // the batch holds the stream's last segment
    uint8_t* dst;                               // the destination (absolute positions)
    uint64_t base, nbytes;                      // the batch's first output byte, its bytes
    uint32_t* st; uint32_t* pend; uint64_t words;   // nbytes pointers, the bitmap's words (zero on entry)
    zz_pt_stat* stat;                           // per segment
    unsigned int* next;                         // the next segment to deal out (zero on entry)
    unsigned long long* tot;                    // [ZZ_TOT_FAILED] failed segments
};

// zi_out_segment's bits on the device: set by an atomic (lanes, and the neighbouring segments, share words), read past the L1
// (the atomics work in the L2, so a line this CU's L1 holds may not show them)
struct zz_pt_bits {
    __device__ __forceinline__ void set(zi_view<uint32_t>& m, uint64_t q) const { atomicOr(&m.p[q >> 5], 1u << (q & 31)); }
    __device__ __forceinline__ bool test(const zi_view<uint32_t>& m, uint64_t q) const
    {
        return ((__hip_atomic_load(&m.p[q >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (q & 31)) & 1u) != 0;
    }
};

__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_segments(zz_pt_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        // lane 0 draws the segment, every lane gets its number
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(Q.next, 1u);
        i = uniform(i);
        if (i >= Q.nseg) break;
        const uint64_t b0 = Q.rows[2 * i], o0 = Q.rows[2 * i + 1], b1 = Q.rows[2 * i + 2], o1 = Q.rows[2 * i + 3];
        S.kind = 0;
        const zi_view<const uint8_t> view{ Q.s, Q.sn };
        zz_inf_in in{ Q.s, Q.sn, (uint8_t*)ibuf4, -(int64_t)(2 * ZZ_INF_IBUF), lane };
        zi_out_segment<zz_inf_fence, zz_pt_bits> o{ zi_view<uint8_t>{ Q.dst + o0, o1 - o0 }, zi_view<uint32_t>{ Q.pend, Q.words },
                                                    zi_view<uint32_t>{ Q.st, Q.nbytes }, o0, o0 - Q.base, 0, 0, false, lane,
                                                    ZZ_INF_THREADS, {}, {} };
        zi_pt_segment pt{ (uint32_t)(b0 & 7), b1, Q.last && i + 1 == Q.nseg, 0 };
        const zi_result R = zi_run(in, view, b0 >> 3, o, S, ZI_RUN_POINT, o1 - o0, lane, ZZ_INF_THREADS, pt);
        if (lane == 0) {
            Q.stat[i] = zz_pt_stat{ pt.end_bit, R.err ? 0u : (1u | (R.final ? 2u : 0u)), (uint32_t)R.out };
            if (R.err) atomicAdd(&Q.tot[ZZ_TOT_FAILED], 1ull);
        }
        __syncthreads();                        // the next segment's first stage overwrites the input buffer
    }
}

// pcnt[t] = prem[t] = pending bytes of tile t (ZI_POINTS_TILE / 32 words each; the bitmap is zero behind the batch's bytes),
// tot[ZZ_TOT_PENDING] += their sum. One workgroup per tile.
__global__ __launch_bounds__(256) void k_points_count(const uint32_t* pend, uint32_t* pcnt, uint32_t* prem, unsigned long long* tot)
{
    __shared__ uint32_t red[256 / ZZ_WAVE];
    const uint32_t t = blockIdx.x, i = threadIdx.x;
    const uint4 w = ((const uint4*)(pend + (uint64_t)t * (ZI_POINTS_TILE / 32)))[i];       // 1024 words: four per thread
    uint32_t n = (uint32_t)(__popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w));
    n = inf_wave_sum(n);
    if ((i & 63) == 0) red[i >> 6] = n;
    __syncthreads();
    if (i == 0) {
        uint32_t sum = 0;
        for (int k = 0; k < 256 / ZZ_WAVE; ++k) sum += red[k];
        pcnt[t] = sum; prem[t] = sum;
        if (sum) atomicAdd(&tot[ZZ_TOT_PENDING], (unsigned long long)sum);
    }
}

}  // namespace zz
