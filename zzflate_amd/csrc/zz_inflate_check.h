// zz_inflate_check.h -- checked range reads (zz_decode_range_checked_device, zz_decode_ranges_checked_device, zz_api.hip) and the
// producer of what they check against (zz_packet_checksums_device): a SIDECAR of one public 32-bit checksum per packet. The rules
// -- public value to partial and back, the widened window, the verdict -- are ZZ_HD functions of zz_inflate_core.h;
// tests/cxx/inflate_checked_harness.cpp runs the same procedure with them on the host.
//
//   producer  zz_checksum.h's per-packet partials of d_data, then k_cks_publish: start-0 partial -> zlib's value
//   per call  k_sidecar_unpack   one thread per entry: zlib's value -> start-0 partial, the packet's length from total_len
//             k_cks_reduce       zz_checksum.h: the partials folded in packet order
//             k_sidecar_verdict  the fold against the stream's trailer; one word for the host. The index proposes, the file decides:
//                                a sidecar that does not fold to the trailer is refused before anything is decoded.
//   per batch / per wave, behind the rounds:
//             k_crc32_stage / k_adler_stage   zz_checksum.h's bodies over the stage through zz_stage_map: a packet's length is what
//                                phase 1 says it produced (the device's `stat` word), never a length the host knows
//             k_stage_check_range / k_stage_check_ranges   one thread per stage packet: zi_checked_packet_bad against the sidecar;
//                                a mismatch is counted in tot[ZZ_TOT_BAD_SUM], or charged to the packet's read as a failed packet
//
// Only the packets a read returns bytes from are summed and compared; look-back packets are not (nothing of them is returned).
// Every kernel reads the sidecar only at [0, packets) -- the host has held the entry count to the index's -- and the stage only
// inside the packets phase 1 wrote.
#pragma once
#include "zz_checksum.h"
#include "zz_inflate.h"

namespace zz {

// ---- the stage as a run of packets: zz_packet_view's third form ----------------------------------------------------------
// Stage packet g lies at B.src + g * packet_size and holds stat[g] >> 3 bytes (0 if it failed); with descriptors (a wave of
// zz_decode_ranges_checked_device), a packet outside its read's widened window counts as empty: it is not summed.
struct zz_stage_map {
    const uint32_t* stat;
    const zi_read_desc* desc;       // null: every packet of the launch is a touched one
    uint32_t npk;                   // stage packets of the launch
};
__device__ __forceinline__ uint32_t zz_stage_len(const zz_stage_map& M, uint32_t g, uint32_t P)
{
    const uint32_t s = M.stat[g];
    uint32_t len = (s & 1u) ? s >> 3 : 0u;
    if (len > P) len = P;                               // (phase 1's window is P bytes: cannot happen)
    if (M.desc) { const zi_read_desc d = M.desc[g]; if (d.hi == d.lo) len = 0; }
    return len;
}
__device__ __forceinline__ uint32_t zz_batch_npk(const zz_packet_params&, const zz_stage_map& M) { return M.npk; }
__device__ __forceinline__ zz_packet_params zz_packet_view(const zz_packet_params& B, const zz_stage_map& M, uint32_t g, uint32_t& k)
{
    zz_packet_params P = B;
    k = 0;                                              // the view is a shard of this one packet
    P.src = B.src + (uint64_t)g * B.packet_size;
    P.n = zz_stage_len(M, g, B.packet_size);
    P.npk = 1;
    P.cks = B.cks + g;
    return P;
}

// Adler-32 partials through a MAP (k_adler_packets is the single-stream form): one wavefront per packet, grid-stride
template <class MAP>
__device__ __forceinline__ void adler_packets_run(const zz_packet_params& P0, const MAP& M)
{
    for (uint32_t g = blockIdx.x; g < zz_batch_npk(P0, M); g += gridDim.x) {
        uint32_t k;
        decltype(auto) P = zz_packet_view(P0, M, g, k);
        const uint64_t off = (uint64_t)k * P.packet_size;
        const uint32_t len = (uint32_t)((P.n - off) < P.packet_size ? (P.n - off) : P.packet_size);
        const zz_cks c = wave_adler(P.src + off, len);
        if (lane_id() == 0) P.cks[k] = c;
    }
}
__global__ __launch_bounds__(ZZ_WAVE) void k_adler_stage(zz_packet_params B, zz_stage_map M) { adler_packets_run(B, M); }
__global__ __launch_bounds__(ZZ_CRC_THREADS) void k_crc32_stage(zz_packet_params B, zz_stage_map M) { crc32_packets_run(B, M); }

// ---- the producer's conversion: partials of n bytes in packets of P -> the sidecar ------------------------------------------
__global__ __launch_bounds__(256) void k_cks_publish(const zz_cks* part, uint32_t npk, uint32_t P, uint64_t n, int kind, uint32_t* out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npk) return;
    const zz_cks c = part[k];
    out[k] = zi_cks_public(kind, c.a, c.b, zi_sidecar_len(k, n, P));
}

// ---- the sidecar against the stream's trailer ----------------------------------------------------------------------------
// verdict[0]: 1 = the sidecar folds to the trailer; verdict[1]: entries no packet of their length can have (zeroed by the host)
__global__ __launch_bounds__(256) void k_sidecar_unpack(const uint32_t* cks, uint32_t npk, uint32_t P, uint64_t L, int kind, zz_cks* part,
                                                        uint32_t* verdict)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npk) return;
    zz_cks c;
    if (!zi_cks_partial(kind, cks[k], zi_sidecar_len(k, L, P), &c.a, &c.b)) atomicAdd(&verdict[1], 1u);
    part[k] = c;
}
__global__ void k_sidecar_verdict(const uint8_t* trailer, int format, const zz_cks_total* fold, uint64_t L, uint32_t* verdict)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    verdict[0] = (verdict[1] == 0 && zi_sidecar_trailer_ok(format, trailer, fold->a, fold->b, L)) ? 1u : 0u;
}

// ---- the stage against the sidecar -----------------------------------------------------------------------------------------
struct zz_chk_params {
    const uint32_t* cks; uint64_t npk; uint64_t L; uint32_t P; int kind;       // the sidecar, the stream's packets and decoded length
    const zz_cks* part; const uint32_t* stat;                                  // per stage packet of the launch: its sum, phase 1's word
};
__device__ __forceinline__ bool stage_packet_bad(const zz_chk_params& C, uint32_t j, uint64_t k)
{
    const uint32_t s = C.stat[j];
    if (!(s & 1u)) return true;                                                // it did not decode
    const zz_cks c = C.part[j];
    return zi_checked_packet_bad(C.kind, c.a, c.b, s >> 3, C.cks[k], k, C.npk, C.L, C.P);
}
// single read: stage packets [0, n) of the launch are the stream's packets [k_first, k_first + n), all of them touched
__global__ __launch_bounds__(256) void k_stage_check_range(zz_chk_params C, uint64_t k_first, uint32_t n, unsigned long long* bad)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (stage_packet_bad(C, j, k_first + j)) atomicAdd(bad, 1ull);
}
// a wave of reads: a stage packet finds its stream packet and its read through its descriptor. A read that has external bytes in
// its (widened) window repeats, so its sums mean nothing and are not charged; the rounds are over, its count is final.
__global__ __launch_bounds__(256) void k_stage_check_ranges(zz_chk_params C, const zi_read_desc* desc, uint32_t n, zi_read* reads)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const zi_read_desc D = desc[j];
    if (D.hi == D.lo || reads[D.read].ext != 0) return;
    if (stage_packet_bad(C, j, D.k)) atomicAdd(&reads[D.read].fail, 1u);
}

}  // namespace zz
