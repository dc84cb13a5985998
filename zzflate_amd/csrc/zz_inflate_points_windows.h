// zz_inflate_points_windows.h -- the window sidecar of a point index built on the device (zz_points_windows_device, zz_api.hip). The
// rules -- where a slot's bytes lie on the stage, its zero front, a segment's sum, the superset walk, the thinning -- are ZZ_HD
// functions of zz_inflate_core.h (zi_pw_*, zi_points_superset, zi_points_thin); tests/cxx/points_windows_harness.cpp runs the same
// procedure with them on the host.
//
// A batch of whole sidecar segments is decoded by zz_inflate_points.h's three kernels, unchanged, onto a stage: 32 KiB carried from
// the batch before and then the batch, or the caller's destination. They address the destination by absolute position, so they are
// handed the pointer position 0 would have. New here:
//
//   cut      k_points_windows_cut     k_inflate_segments' shape: one wavefront per workgroup, persistent, the batch's sidecar segments
//                                     dealt from a counter. For segment k the wavefront copies slot k -- the 32 KiB in front of
//                                     out_byte[k]: carried bytes, the batch's, or both; zeros in front where the stream is shorter --
//                                     and sums the segment's resolved bytes (zi_adler_lanes / zi_crc_lanes, as
//                                     k_inflate_segments_win sums its slot). One more item, when the stream goes on: the slot of the
//                                     NEXT batch's first segment, which one device-to-device copy makes the next carry. No LDS.
//
// A sidecar segment longer than the stage (possible only when the decode rows are finer than the sidecar's) is cut in pieces: the
// same kernel over the two ends of a piece, its slots written to a spare place, the pieces' sums joined on the host (zi_pr_join).
//
// Bounds: the host has checked the rows (zi_points_check) and planned the batch over them, so out_byte ascends inside
// [base, base + nbytes]; a slot reads buf[at, at + 32768 - zeros) with at = out_byte - have - org >= 0 and at + have <= 32768 + nbytes
// (org = base - 32768) or <= out_byte <= cap (org = 0), and writes its own 32768 bytes of d_windows; a sum reads its segment's bytes.
#pragma once
#include "zz_inflate_points.h"

namespace zz {

struct zz_pw_params {
    const uint8_t* buf; uint64_t buf_n;         // the stage (or the destination up to the unit's end)
    int64_t org;                                // absolute output position of buf[0] (zi_pw_org)
    const uint64_t* rows;                       // the rows to cut at: nseg + 1 of them
    uint32_t nseg;
    uint8_t* windows; uint32_t* sums;           // slot i and sum i of the segment behind row i, i < nseg
    uint8_t* tail;                              // the slot of row nseg: the next carry (null: none)
    int kind;                                   // ZI_CKS_ADLER or ZI_CKS_CRC
    unsigned int* next;                         // the next item to deal out (zero on entry)
};

__global__ __launch_bounds__(ZZ_INF_THREADS) void k_points_windows_cut(zz_pw_params Q)
{
    const uint32_t lane = threadIdx.x;
    zz_inf_lanes w{ nullptr, lane };
    const zi_view<const uint8_t> buf{ Q.buf, Q.buf_n };
    for (;;) {
        // lane 0 draws the item, every lane gets its number
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(Q.next, 1u);
        i = uniform(i);
        if (i >= Q.nseg + (Q.tail ? 1u : 0u)) break;
        const uint64_t o0 = Q.rows[2 * i + 1];
        uint8_t* const slot = i < Q.nseg ? Q.windows + (uint64_t)i * ZI_PR_WINDOW : Q.tail;
        zi_pw_slot_copy(buf, zi_view<uint8_t>{ slot, ZI_PR_WINDOW }, zi_pw_slot_place(o0, Q.org), lane, ZZ_INF_THREADS);
        if (i < Q.nseg) {
            const uint32_t sum = zi_pw_segment_sum(w, Q.kind, buf, Q.org, o0, Q.rows[2 * i + 3], lane, ZZ_INF_THREADS);
            if (lane == 0) Q.sums[i] = sum;
        }
        // every lane arrives here before lane 0 draws again: without the barrier the compiler threads `lane == 0` across the back
        // edge, lane 0 leaves for the store and the draw, and the other lanes read "the first lane's" number without it
        __syncthreads();
    }
}

}  // namespace zz
