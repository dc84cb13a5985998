// zz_inflate_members_decode.h -- decode of a file of LARGE gzip members in parallel from its member point index
// (zz_decode_members_points_device, zz_api.hip): many wavefronts per member, where zz_decode_members_found_device has one. The rules
// -- zi_mpd_plan, zi_mpd_mstar, zi_mpd_batch, zi_mpd_segment, zi_mpd_fold_run / _step, zi_mpd_verdict -- are ZZ_HD functions of
// zz_inflate_core.h, and tests/cxx/members_points_decode_harness.cpp runs the same procedure with them on the host.
//
//   phase 1  k_members_segments   k_inflate_segments' shape with a descriptor per segment (zi_mpd_seg, made by the host while it checks
//                                 the rows): one wavefront per workgroup, persistent, the batch's descriptors dealt from a counter. The
//                                 view is the FILE, the destination is addressed by absolute position, and a distance that reaches in
//                                 front of the member's first byte is an error, not a pending byte: pointers never leave their member.
//   count    k_points_count       zz_inflate_points.h's, unchanged
//   phase 2  k_inflate_resolve    zz_inflate.h's rounds, unchanged
//   sums     k_members_sums       per batch, behind its rounds: one wavefront per segment, the CRC-32 of its bytes (zi_crc_lanes) into
//                                 a per-file array of 4 bytes per segment
//   verdict  k_members_verdict    once, behind the last batch: one wavefront per dealt member. A lane joins a run of consecutive
//                                 segment sums, a tree over the 64 lanes joins the runs in order, lane 0 holds the member to its
//                                 header, its trailer's CRC-32 and ISIZE and its segments' flags, writes status[j] and lowers first_bad.
//   tail     k_inflate_members    zz_inflate_members.h's, unchanged: from the first member that is not proven
//
// What keeps these kernels from hanging, by construction: one wavefront per workgroup, so a barrier is met by the 64 lanes that
// met the one before; no kernel waits for another workgroup (no flag, no spin: order comes from the launches on the stream); and
// every loop ends on a bound that decoded data cannot move -- the dealing loops on i >= n, zi_run on its view (the file's length),
// the fold on the member's segment count, the tree on six steps.
//
// Every kernel reads only the file src[0, n), the destination inside [0, cap) and its workspace; phase 1 writes only its segment's
// bytes of the destination (zi_out_segment's capacity is the segment's announced length, and a dealt member ends inside cap).
#pragma once
#include "zz_inflate_points.h"

namespace zz {

#define ZZ_MPD_WG_PER_CU 16                     // resident workgroups (= wavefronts) per CU the grids are sized for

struct zz_mpd_params {
    const uint8_t* src; uint64_t n;             // the file
    const zi_mpd_seg* seg;                      // the dealt descriptors of the call
    uint64_t k0; uint32_t nseg;                 // this batch: descriptors [k0, k0 + nseg)
    uint8_t* dst;                               // the destination (absolute positions)
    uint64_t base, nbytes;                      // the batch's first output byte, its bytes
    uint32_t* st; uint32_t* pend; uint64_t words;   // nbytes pointers, the bitmap's words (zero on entry)
    uint8_t* segok;                             // per descriptor of the call: 1 its run was accepted (zero on entry)
    uint32_t* sums;                             // per descriptor of the call: the CRC-32 of its bytes
    unsigned int* next;                         // the next descriptor to deal out (zero on entry)
    unsigned long long* tot;                    // [ZZ_TOT_FAILED] refused segments
};

// The one way the kernels of this file draw work: lane 0 takes the next number from the counter and every lane gets it. Every turn
// BEGINS with the barrier, so none of the three dealing loops can stand without one. It is not only for memory (the next turn's first
// stage overwrites the input buffer, the next member's runs overwrite the verdict's partials): it is what keeps the 64 lanes in the
// loop together. In a loop whose body has a side effect in lane 0 alone and no convergent operation, the compiler lets the other
// lanes leave after the first turn (their own copy of the number folds to 0, so for them the loop never breaks) and parks them in an
// endless loop behind it -- the wavefront never ends.
__device__ __forceinline__ uint32_t mpd_deal(unsigned int* next, uint32_t lane)
{
    __syncthreads();
    uint32_t i = 0;
    if (lane == 0) i = atomicAdd(next, 1u);
    return uniform(i);
}

__global__ __launch_bounds__(ZZ_INF_THREADS) void k_members_segments(zz_mpd_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        const uint32_t i = mpd_deal(Q.next, lane);
        if (i >= Q.nseg) break;
        const zi_mpd_seg d = Q.seg[Q.k0 + i];
        zz_inf_in in{ Q.src, Q.n, (uint8_t*)ibuf4, -(int64_t)(2 * ZZ_INF_IBUF), lane };
        uint32_t np = 0;
        const zi_result R = zi_mpd_segment<zz_inf_fence, zz_pt_bits>(in, Q.src, Q.n, d, Q.dst, Q.base, Q.pend, Q.words, Q.st, Q.nbytes, S,
                                                                     lane, ZZ_INF_THREADS, &np);
        if (lane == 0) {
            Q.segok[Q.k0 + i] = R.err ? 0 : 1;
            if (R.err) atomicAdd(&Q.tot[ZZ_TOT_FAILED], 1ull);
        }
    }
}

// sums[k] = CRC-32 of dst[o0, o1) for the batch's descriptors; one wavefront per segment, persistent
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_members_sums(zz_mpd_params Q)
{
    const uint32_t lane = threadIdx.x;
    zz_inf_lanes w{ nullptr, lane };            // (no input is staged: the lanes read the destination)
    for (;;) {
        const uint32_t i = mpd_deal(Q.next, lane);
        if (i >= Q.nseg) break;
        const zi_mpd_seg d = Q.seg[Q.k0 + i];
        const uint64_t len = d.o1 - d.o0;
        const uint32_t c = zi_crc_lanes(w, zi_view<const uint8_t>{ Q.dst + d.o0, len }, len, lane, ZZ_INF_THREADS);
        if (lane == 0) Q.sums[Q.k0 + i] = c;
    }
}

struct zz_mpd_verdict_params {
    const uint8_t* src; uint64_t n;
    const zi_mpd_member* mem; uint32_t nmem;    // the dealt members
    const zi_mpd_seg* seg; const uint32_t* sums; const uint8_t* segok;
    uint8_t* status;                            // per dealt member: 1 proven
    unsigned long long* first_bad;              // the first dealt member that is not proven (nmem or more on entry)
    unsigned int* next;                         // the next member to deal out (zero on entry)
};
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_members_verdict(zz_mpd_verdict_params Q)
{
    __shared__ zi_pr_part part[ZZ_INF_THREADS];
    const uint32_t lane = threadIdx.x;
    for (;;) {
        const uint32_t j = mpd_deal(Q.next, lane);
        if (j >= Q.nmem) break;
        const zi_mpd_member M = Q.mem[j];
        bool ok = true;
        part[lane] = zi_mpd_fold_run(M, Q.seg, Q.sums, Q.segok, lane, ZZ_INF_THREADS, &ok);
        const bool all_ok = __all(ok) != 0;
        for (uint32_t o = 1; o < ZZ_INF_THREADS; o <<= 1) {    // six steps
            __syncthreads();
            zi_mpd_fold_step(part, lane, ZZ_INF_THREADS, o);
        }
        __syncthreads();
        if (lane == 0) {
            const bool proven = zi_mpd_verdict(Q.src, Q.n, M, part[0], all_ok);
            Q.status[j] = proven ? 1 : 0;
            if (!proven) atomicMin(Q.first_bad, (unsigned long long)j);
        }
    }
}

}  // namespace zz
