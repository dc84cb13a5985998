// zz_inflate_members_points.h -- one index over the members of a file AND the blocks inside them, built on the device
// (zz_members_points_device, zz_api.hip): the cuts a decode of files whose members are large -- `cat lane1.fq.gz lane2.fq.gz`,
// rotated logs joined with cat -- needs to use many wavefronts per member. The rules -- zi_mp_measure, zi_mp_link, zi_mp_rows,
// zi_mp_to_index -- are ZZ_HD functions of zz_inflate_core.h, and
// tests/cxx/members_points_harness.cpp runs the same procedure with them on the host.
//
//   mark     k_members_find_mark, k_members_scan   zz_inflate_members_find.h's, unchanged: the header candidates H
//            k_points_find                         zz_inflate_points_find.h's, unchanged, with D = the file: the block candidates B
//   reach    k_members_points_reach   k_points_reach's shape: one wavefront per workgroup, persistent, the round's jobs dealt from a
//                                     counter, sixteen workgroups per CU. A job is zi_mp_measure: a header job parses its header first,
//                                     either kind finds its stop among the block candidates, counts to it (or through a final block,
//                                     then reads ISIZE) and writes its 40-byte record and nothing else.
// The walk over the jobs' records (zi_mp_link) runs on the host, as zi_find_link and zi_mf_link do.
//
// Every kernel reads only [src, src + n) and its workspace and writes only its records.
#pragma once
#include "zz_inflate_members_find.h"
#include "zz_inflate_points_find.h"

namespace zz {

#define ZZ_MP_WG_PER_CU 16

struct zz_mp_params {
    const uint8_t* src; uint64_t n;
    const uint64_t* bc; uint64_t nb;            // the block candidates, ascending
    uint64_t chunk;                             // chunk_bytes: a limited job gives up that far behind its stop
    zi_mp_job* job; uint32_t njobs;             // the round's jobs, results in place
    unsigned int* next;                         // the next job to deal out (zero on entry)
};
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_members_points_reach(zz_mp_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    zz_inf_lanes w{ (uint8_t*)ibuf4, lane };
    const zi_view<const uint64_t> bc{ Q.bc, Q.nb };
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(Q.next, 1u);
        i = uniform(i);
        if (i >= Q.njobs) break;
        const zi_mp_job j = Q.job[i];
        const zi_mp_job r = zi_mp_measure(w, Q.src, Q.n, bc, Q.nb, Q.chunk, 0, j, S, lane, ZZ_INF_THREADS);
        if (lane == 0) Q.job[i] = r;
        __syncthreads();                        // the next job's first stage overwrites the input buffer
    }
}

}  // namespace zz
