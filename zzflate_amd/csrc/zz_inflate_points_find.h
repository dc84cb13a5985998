// zz_inflate_points_find.h -- the point index of ANY zlib / gzip / raw stream built on the device (zz_points_index_device, zz_api.hip;
// the rules -- zi_find_prefilter, zi_find_header, zi_out_count, ZI_RUN_REACH, zi_find_link, zi_find_rows -- are in zz_inflate_core.h,
// and tests/cxx/points_find_harness.cpp runs them on the CPU).
//
//   find   k_points_find    one wavefront per workgroup, persistent, the chunks c >= 1 of D dealt from a counter (the shape of
//                           k_inflate_segments). The chunk goes through the LDS in tiles of ZZ_PF_TILE bytes; every step the 64
//                           lanes prefilter 64 consecutive bit positions (eight bytes) out of the tile, and the survivors
//                           (a ballot) are put to the full test in ascending order by the whole wavefront: zi_find_header over the
//                           ordinary staged input, which reads past the chunk's end as far as D goes and zeros behind it. The
//                           first position that passes is the chunk's candidate: job[c].a, or ZI_FIND_NONE. The tile and the
//                           staged input share one 2 KiB buffer (a full test is rare, and the tile is staged again behind it), so
//                           the LDS is k_inflate_segments': the tables and 2 KiB.
//   reach  k_points_reach   one wavefront per workgroup, persistent, the round's jobs dealt from a counter. A job is
//                           zi_run<zi_out_count, zi_pt_reach> from its bit: it counts, and writes nothing but its 32-byte record.
//                           All jobs of a round are one launch, whatever the stream's decoded length.
//
// The chain over the jobs' records (zi_find_link, zi_find_rows) is walked on the host, which reads the records of a round -- 32
// bytes per job -- and sends the repair jobs of the next; no workgroup waits for another.
//
// Every kernel reads only D = d[0, n) and its records and writes only its records.
#pragma once
#include "zz_inflate.h"

namespace zz {

#define ZZ_PF_TILE (ZZ_INF_IBUF - 32)           // bytes of a tile whose bit positions are searched; the 32 behind them are read only
#define ZZ_PF_WG_PER_CU 16

struct zz_pf_params {
    const uint8_t* d; uint64_t n;               // D: the DEFLATE bytes and the trailer
    uint64_t chunk, chunks;                     // find: chunk_bytes, zi_find_chunks(n, chunk)
    zi_find_job* job;                           // find: one per chunk (a = the candidate); reach: the round's jobs, results in place
    uint32_t njobs;                             // reach
    unsigned int* next;                         // the next chunk / job to deal out (zero on entry)
};

// the tile as a byte source: bytes [t0, t0 + ZZ_INF_IBUF) of D at buf, zeros behind D
struct zz_pf_tile {
    const uint8_t* buf; uint64_t t0;
    __device__ __forceinline__ uint64_t peek8(uint64_t pos) const
    {
        const uint32_t off = (uint32_t)(pos - t0);
        const uint32_t* w = (const uint32_t*)buf + (off >> 2);
        const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
        const uint32_t sh = (off & 3) * 8;
        return sh ? (lo >> sh) | ((uint64_t)w[2] << (64 - sh)) : lo;
    }
};

__global__ __launch_bounds__(ZZ_INF_THREADS) void k_points_find(zz_pf_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    uint8_t* const buf = (uint8_t*)ibuf4;
    const uint32_t lane = threadIdx.x;
    const zi_view<const uint8_t> view{ Q.d, Q.n };
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(Q.next, 1u);
        c = uniform(c) + 1;                                       // chunk 0's candidate is bit 0
        if (c >= Q.chunks) break;
        const uint64_t b0 = (uint64_t)c * Q.chunk;
        const uint64_t b1 = b0 + Q.chunk < Q.n ? b0 + Q.chunk : Q.n;            // the chunk's bytes [b0, b1)
        uint64_t found = ZI_FIND_NONE;
        for (uint64_t t0 = b0; t0 < b1 && found == ZI_FIND_NONE; t0 += ZZ_PF_TILE) {
            bool staged = false;
            const uint64_t t1 = t0 + ZZ_PF_TILE < b1 ? t0 + ZZ_PF_TILE : b1;
            for (uint64_t at = t0; at < t1 && found == ZI_FIND_NONE; at += 8) {
                if (!staged) {
                    __syncthreads();                                             // every lane is done with what the buffer held
                    for (uint32_t i = lane; i < ZZ_INF_IBUF / 4; i += ZZ_INF_THREADS) {
                        const uint64_t q = t0 + 4ull * i;
                        uint32_t v = 0;
                        if (q + 4 <= Q.n) v = load32(Q.d + q);
                        else for (uint32_t k = 0; k < 4; ++k) if (q + k < Q.n) v |= (uint32_t)Q.d[q + k] << (8 * k);
                        ((uint32_t*)buf)[i] = v;
                    }
                    __syncthreads();
                    staged = true;
                }
                const uint64_t p = at * 8 + lane;                                // lane l: byte at + l / 8, bit l % 8
                zz_pf_tile tile{ buf, t0 };
                const bool pre = p < t1 * 8 && zi_find_prefilter_at(tile, p);
                uint64_t m = ballot(pre);
                while (m) {                                                      // rare: the whole wavefront tests one position
                    const uint32_t l = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    __syncthreads();
                    zz_inf_in in{ Q.d, Q.n, buf, -(int64_t)(2 * ZZ_INF_IBUF), lane };
                    staged = false;
                    if (zi_find_header(in, view, at * 8 + l, S, lane, ZZ_INF_THREADS)) { found = at * 8 + l; break; }
                }
            }
        }
        if (lane == 0) Q.job[c].a = found;
        __syncthreads();
    }
}

__global__ __launch_bounds__(ZZ_INF_THREADS) void k_points_reach(zz_pf_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    const zi_view<const uint8_t> view{ Q.d, Q.n };
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(Q.next, 1u);
        i = uniform(i);
        if (i >= Q.njobs) break;
        const zi_find_job j = Q.job[i];
        zz_inf_in in{ Q.d, Q.n, (uint8_t*)ibuf4, -(int64_t)(2 * ZZ_INF_IBUF), lane };
        const zi_find_job r = zi_find_reach(in, view, j, S, lane, ZZ_INF_THREADS);
        if (lane == 0) Q.job[i] = r;
        __syncthreads();                        // the next job's first stage overwrites the input buffer
    }
}

}  // namespace zz
