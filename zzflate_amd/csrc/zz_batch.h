// zz_batch.h -- many independent streams in one call (zz_encode_batch_device). Item i = srcs[i][0, ns[i]) becomes the stream
// zz_encode_device would write for it alone: container header, its packets (cold, byte-aligned, zzflate.cpp:101-125), trailer.
//
//   plan      k_batch_plan     per item: packets and slot bytes, exclusive scans over the items -> first[], slotbase[], totals
//             k_batch_desc     per packet: {item, packet within the item, slot offset} (binary search over first[])
//             k_batch_tails    per item: its 128-byte tail (k_fill_tail of one shard)
//   encode    the batch forms of the packet kernels: the single-stream bodies, each packet seeing its item through
//             zz_packet_view (zz_common.h) -- its src, end, tail, final flag, slot, size and checksum entries; with the
//             call's extended switch, levels 4..6 on k_l6_matches_batch (zz_level6.h) and k_encode_l2x_batch, the window
//             of a packet being the bytes of its own item in front of it and nothing else
//   join      k_scan_sizes     one exclusive scan over all packets: a packet's offset in its item is the difference to the
//                              item's first packet (a segmented scan by subtraction)
//             k_batch_finalize one wavefront per item: stream bytes, the checksum fold over its packets, room check, header,
//                              trailer, out_lens[i] (~0 when it does not fit)
//             k_batch_compact  one wavefront per packet: slot -> dsts[item] + header + offset, for items that fit
//
// Slots are sized by the packet's own length (zz_slot_stride(level, len)), so the workspace follows the batch's bytes, not
// its item count times a full packet's slot.
#pragma once
#include "zz_level0.h"
#include "zz_level1.h"
#include "zz_level1p.h"
#include "zz_level2.h"
#include "zz_compact.h"

namespace zz {

struct zz_batch_totals {
    uint64_t npk;            // packets of the batch (the plan)
    uint64_t slot_bytes;     // bytes of slots they need (the plan)
    uint64_t nospace;        // items that did not fit their destination (the join)
};

__device__ __forceinline__ uint32_t batch_header_len(int format) { return format == ZZ_FMT_ZLIB ? 2 : format == ZZ_FMT_GZIP ? 10 : 0; }
__device__ __forceinline__ uint32_t batch_trailer_len(int format) { return format == ZZ_FMT_ZLIB ? 4 : format == ZZ_FMT_GZIP ? 8 : 0; }

// ---- plan -------------------------------------------------------------------------------------------------------------
// One workgroup, ZZ_BATCH_PLAN_PER items per thread and round. first[] is 32-bit: the host refuses totals above 2^31 - 1
// before anything reads it.
#define ZZ_BATCH_PLAN_PER 8
__global__ __launch_bounds__(ZZ_SCAN_THREADS) void k_batch_plan(const uint64_t* ns, uint32_t nitems, uint32_t P, int level,
                                                                uint32_t* first, uint64_t* slotbase, zz_batch_totals* out)
{
    __shared__ uint64_t wc[ZZ_SCAN_THREADS / ZZ_WAVE], wb[ZZ_SCAN_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    const uint32_t full = level ? zz_slot_stride(level, P) : 0;
    uint64_t carry_c = 0, carry_b = 0;
    for (uint64_t r0 = 0; r0 < nitems; r0 += (uint64_t)ZZ_BATCH_PLAN_PER * ZZ_SCAN_THREADS) {
        const uint64_t i0 = r0 + (uint64_t)t * ZZ_BATCH_PLAN_PER;
        uint64_t cnt[ZZ_BATCH_PLAN_PER], sb[ZZ_BATCH_PLAN_PER], tc = 0, tb = 0;
#pragma unroll
        for (int u = 0; u < ZZ_BATCH_PLAN_PER; ++u) {
            const uint64_t n = i0 + u < nitems ? ns[i0 + u] : 0;
            const uint64_t npk = (n + P - 1) / P;
            cnt[u] = npk;
            sb[u] = (npk && level) ? (npk - 1) * full + zz_slot_stride(level, (uint32_t)(n - (npk - 1) * P)) : 0;
            tc += cnt[u]; tb += sb[u];
        }
        const wg_prefix2<uint64_t, uint64_t> s = wg_scan_excl2<ZZ_SCAN_THREADS>(tc, wc, tb, wb, carry_c, carry_b);      // packets, slot bytes
        uint64_t bc = s.a.excl, bb = s.b.excl;
#pragma unroll
        for (int u = 0; u < ZZ_BATCH_PLAN_PER; ++u) {
            if (i0 + u < nitems) { first[i0 + u] = (uint32_t)bc; slotbase[i0 + u] = bb; }
            bc += cnt[u]; bb += sb[u];
        }
        carry_c += s.a.total; carry_b += s.b.total;
        __syncthreads();
    }
    if (t == 0) {
        first[nitems] = (uint32_t)carry_c;
        out->npk = carry_c;
        out->slot_bytes = carry_b;
        out->nospace = 0;
    }
}

// one thread per packet: the item is the last one whose first packet is at or below g (empty items share their successor's
// first packet and are skipped by the search)
__global__ __launch_bounds__(256) void k_batch_desc(const uint32_t* first, uint32_t nitems, uint32_t npk, uint32_t P, int level,
                                                    const uint64_t* slotbase, zz_batch_desc* desc)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= npk) return;
    uint32_t lo = 0, hi = nitems;                          // first[lo] <= g < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    zz_batch_desc d;
    d.item = lo;
    d.k = g - first[lo];
    d.slot = slotbase[lo] + (uint64_t)d.k * zz_slot_stride(level, P);
    desc[g] = d;
}

// the batch's k_fill_tail: one workgroup of 128 threads per item
__global__ __launch_bounds__(128) void k_batch_tails(const uint8_t* const* srcs, const uint64_t* ns, uint32_t nitems, uint8_t* tails)
{
    for (uint32_t i = blockIdx.x; i < nitems; i += gridDim.x) {
        const uint64_t n = ns[i];
        const uint64_t tn = n < 64 ? n : 64;
        const uint32_t b = threadIdx.x;
        tails[(uint64_t)i * 128 + b] = b < tn ? srcs[i][n - tn + b] : (uint8_t)0;
    }
}

// ---- the batch forms of the packet kernels ------------------------------------------------------------------------------
struct zz_l0_batch_params {
    zz_packet_params pk;     // packet_size, cks_kind, cks (per packet of the batch)
    uint8_t* const* dsts;    // per item: its destination
    const uint64_t* caps;    // per item: its capacity
    int format;
};
__host__ __device__ inline uint64_t l0_item_bytes(uint64_t n, uint32_t P)
{
    if (n == 0) return 5;                                  // one empty stored final block
    const uint64_t npk = (n + P - 1) / P;
    return (npk - 1) * l0_packet_bytes(P, false) + l0_packet_bytes((uint32_t)(n - (npk - 1) * P), true);
}
// level 0 writes straight into the item's destination, where it fits (the room check per item, on the device)
__global__ __launch_bounds__(256) void k_encode_l0_batch(zz_l0_batch_params Q, zz_batch_map M)
{
    __shared__ uint64_t red_a[4], red_c[4];
    const uint32_t hl = batch_header_len(Q.format), tl = batch_trailer_len(Q.format);
    for (uint32_t g = blockIdx.x; g < M.npk; g += gridDim.x) {
        uint32_t k;
        const zz_packet_params P = zz_packet_view(Q.pk, M, g, k);
        const uint32_t item = M.desc[g].item;
        if (hl + l0_item_bytes(P.n, P.packet_size) + tl > Q.caps[item]) continue;     // (uniform: the whole workgroup skips)
        uint8_t* d = Q.dsts[item] + hl + (uint64_t)k * l0_packet_bytes(P.packet_size, false);
        l0_encode_packet(P, k, d, 0, red_a, red_c);
    }
}

__global__ __launch_bounds__(ZZ_L1_THREADS) void k_encode_l1_batch(zz_packet_params B, zz_batch_map M)
{
    __shared__ uint16_t T[ZZ_HASH_SIZE];
    __shared__ uint32_t ring_words[ZZ_RING_WORDS];
    __shared__ __attribute__((aligned(512))) uint32_t tokbuf[2 * ZZ_L1_TOKSLOT];
    uint32_t k;
    const zz_packet_params P = zz_packet_view(B, M, blockIdx.x, k);
    if (uniform(threadIdx.x >> 6) == 0) l1_packet_parser<0>(P, k, T, tokbuf);
    else l1_packet_emitter(P, k, ring_words, tokbuf);
}

__global__ __launch_bounds__(ZZ_L1P_THREADS) void k_encode_l1p_batch(zz_packet_params B, zz_batch_map M)
{
    __shared__ uint16_t T[ZZ_HASH_SIZE];
    __shared__ uint32_t ring_words[ZZ_RING_WORDS];
    __shared__ __attribute__((aligned(512))) uint32_t tokbuf[2 * ZZ_L1_TOKSLOT];
    __shared__ l1p_xch X;
    uint32_t k;
    const zz_packet_params P = zz_packet_view(B, M, blockIdx.x, k);
    const uint32_t wv = uniform(threadIdx.x >> 6);
    if (wv < 2) l1p_packet_parser<0u>(P, k, T, tokbuf, &X, wv);
    else l1p_packet_emitter<0u>(P, k, ring_words, tokbuf);
}

// levels 2,3: PP = the two-parser form (k_encode_l2p); Q.k0 = 0, Q.k1 = the batch's packets
template <bool PP>
__global__ __launch_bounds__(PP ? ZZ_L2P_THREADS : ZZ_L2_THREADS, PP ? ZZ_L2P_WPE : 5) void k_encode_l2_batch_t(zz_l2_params Q, zz_batch_map M)
{
    l2_encode_run<0u, false, PP>(Q, M);
}

// the extended levels 4..6: the parser reads k_l6_matches_batch's words (the row of m is the batch's packet number's), package-merge codes
__global__ __launch_bounds__(ZZ_L2_THREADS, 6) void k_encode_l2x_batch(zz_l2_params Q, zz_batch_map M)
{
    l2_encode_run<32768u, true, false>(Q, M);
}

__global__ __launch_bounds__(ZZ_CRC_THREADS) void k_crc32_packets_batch(zz_packet_params B, zz_batch_map M) { crc32_packets_run(B, M); }

// ---- join ---------------------------------------------------------------------------------------------------------------
struct zz_batch_join {
    zz_batch_map map;
    const uint32_t* sizes;   // per packet (levels >= 1)
    const uint64_t* offsets; // per packet: exclusive scan of sizes over the whole batch (levels >= 1)
    const zz_cks* cks;       // per packet partials (cks_kind != NONE)
    const uint8_t* slots;
    uint8_t* const* dsts;
    const uint64_t* caps;
    uint64_t* out_lens;
    zz_batch_totals* totals;
    uint32_t nitems;
    uint32_t packet_size;
    int format, cks_kind, level;
};

// The CRC-32 of an item from its packets' partials (cks[k].a: packet k with start value 0), by one wavefront: every lane folds a
// run of packets, then shifts it by the bytes behind the run; the runs XOR together. xp = gf2_xpow8(P).
__device__ __forceinline__ uint32_t batch_crc_fold(const zz_cks* cks, uint32_t npk, uint64_t n, uint32_t P, uint32_t xp, uint32_t lane)
{
    const uint32_t per = (npk + ZZ_WAVE - 1) / ZZ_WAVE;
    uint32_t k0 = lane * per, k1 = k0 + per;
    if (k0 > npk) k0 = npk;
    if (k1 > npk) k1 = npk;
    uint32_t a = 0;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint64_t off = (uint64_t)k * P;
        const uint64_t l = (n - off) < P ? (n - off) : P;
        a = gf2_mulmod(a, l == P ? xp : gf2_xpow8(l)) ^ cks[k].a;
    }
    if (k0 < k1) {
        const uint64_t e = (uint64_t)k1 * P;
        a = gf2_mulmod(a, gf2_xpow8(n - (e < n ? e : n)));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a ^= __shfl_xor(a, o);
    return a;
}

// one wavefront per item: what k_cks_reduce and k_finalize do for one stream
#define ZZ_BATCH_FIN_THREADS 256
__global__ __launch_bounds__(ZZ_BATCH_FIN_THREADS) void k_batch_finalize(zz_batch_join J)
{
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, per_block = ZZ_BATCH_FIN_THREADS / ZZ_WAVE;
    const uint32_t P = J.packet_size;
    const uint32_t hl = batch_header_len(J.format), tl = batch_trailer_len(J.format);
    const uint32_t xp = J.cks_kind == ZZ_CKS_CRC ? gf2_xpow8(P) : 0;
    for (uint32_t i = blockIdx.x * per_block + wv; i < J.nitems; i += gridDim.x * per_block) {
        const uint32_t f = J.map.first[i], npk = J.map.first[i + 1] - f;
        const uint64_t n = J.map.ns[i];
        uint64_t stream;
        if (npk == 0) stream = J.level == 0 ? 5 : 2;                                  // one empty final block (stored / fixed)
        else if (J.level == 0) stream = l0_item_bytes(n, P);
        else stream = J.offsets[f + npk - 1] + J.sizes[f + npk - 1] - J.offsets[f];
        const uint64_t total = hl + stream + tl;
        // the checksum over the item's packets, in order
        uint32_t cks = 0;
        if (J.cks_kind == ZZ_CKS_ADLER) {
            // adler.cpp:5-15 unrolled: A = sum a_k, B = sum b_k + a_k * (bytes after packet k), mod 65521
            uint64_t sA = 0, sB = 0;
            for (uint32_t k = lane; k < npk; k += ZZ_WAVE) {
                const zz_cks c = J.cks[f + k];
                const uint64_t e = (uint64_t)(k + 1) * P;
                const uint32_t r = (uint32_t)((n - (e < n ? e : n)) % ZZ_ADLER_MOD);
                sA += c.a;
                sB += c.b + (uint64_t)c.a * r;
            }
            sA = wave_sum64(sA % ZZ_ADLER_MOD);
            sB = wave_sum64(sB % ZZ_ADLER_MOD);
            const uint32_t part = ((uint32_t)(sB % ZZ_ADLER_MOD) << 16) | (uint32_t)(sA % ZZ_ADLER_MOD);
            cks = adler_combine(1u, part, n);
        } else if (J.cks_kind == ZZ_CKS_CRC) {
            cks = batch_crc_fold(J.cks + f, npk, n, P, xp, lane);
        }
        if (lane == 0) {
            if (total > J.caps[i]) {
                J.out_lens[i] = ~0ull;
                atomicAdd((unsigned long long*)&J.totals->nospace, 1ull);
            } else {
                uint8_t* d = J.dsts[i];
                if (J.format == ZZ_FMT_ZLIB) { d[0] = 0x78; d[1] = 0x01; }              // zzflate.cpp:28-48
                else if (J.format == ZZ_FMT_GZIP) {
                    const uint8_t gz[10] = { 0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xFF };
                    for (int b = 0; b < 10; ++b) d[b] = gz[b];
                }
                if (npk == 0) {
                    uint8_t* e = d + hl;
                    if (J.level == 0) { e[0] = 1; e[1] = 0; e[2] = 0; e[3] = 0xFF; e[4] = 0xFF; }
                    else { e[0] = 0x03; e[1] = 0x00; }
                }
                uint8_t* t = d + hl + stream;                                          // zzflate.cpp:170-192
                if (J.format == ZZ_FMT_ZLIB) {
                    t[0] = (uint8_t)(cks >> 24); t[1] = (uint8_t)(cks >> 16); t[2] = (uint8_t)(cks >> 8); t[3] = (uint8_t)cks;
                } else if (J.format == ZZ_FMT_GZIP) {
                    const uint32_t l = (uint32_t)n;
                    t[0] = (uint8_t)cks; t[1] = (uint8_t)(cks >> 8); t[2] = (uint8_t)(cks >> 16); t[3] = (uint8_t)(cks >> 24);
                    t[4] = (uint8_t)l; t[5] = (uint8_t)(l >> 8); t[6] = (uint8_t)(l >> 16); t[7] = (uint8_t)(l >> 24);
                }
                J.out_lens[i] = total;
            }
        }
    }
}

// one wavefront per packet (a batch of small items has many small packets): slot -> the item's destination, for the items that
// fit (k_batch_finalize has decided: out_lens[item] != ~0)
#define ZZ_BATCH_COMPACT_THREADS 256
__global__ __launch_bounds__(ZZ_BATCH_COMPACT_THREADS) void k_batch_compact(zz_batch_join J)
{
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, per_block = ZZ_BATCH_COMPACT_THREADS / ZZ_WAVE;
    const uint32_t hl = batch_header_len(J.format);
    for (uint32_t g = blockIdx.x * per_block + wv; g < J.map.npk; g += gridDim.x * per_block) {
        const zz_batch_desc d = J.map.desc[g];
        if (J.out_lens[d.item] == ~0ull) continue;
        const uint32_t f = g - d.k;
        coop_copy(J.dsts[d.item] + hl + (J.offsets[g] - J.offsets[f]), J.slots + d.slot, J.sizes[g], lane, ZZ_WAVE);
    }
}

}  // namespace zz
