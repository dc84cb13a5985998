// zz_members_write.h -- one buffer to a blocked gzip (BGZF) file (zz_encode_members_device): what bgzip, samtools and tabix read,
// what zz_decode_members_device decodes in parallel, and what `cat` joins.
//
// The format rule. src[0, n) is cut into blocks of B bytes (the last one shorter; n == 0: none). Member i is
//   header   1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 <BSIZE lo> <BSIZE hi>      BSIZE = the member's bytes - 1
//   body     the raw-deflate stream zz_encode_batch_device(ZZ_DEFLATE, level, P) writes for block i alone (cold packets, the
//            last one final, nothing reaching in front of the block), D bytes -- or, if D > S, the level-0 stream of the same
//            block at the same packet size, S = l0_item_bytes(block, P) bytes (the stored fallback)
//   trailer  CRC-32 of the block, ISIZE, little-endian
// so a member is 26 + min(D, S) bytes and never longer than its stored form; the call refuses (B, P) whose full stored member
// would pass 65,536 bytes (mw_geometry_ok). Behind the last member comes bgzip's empty member of 28 bytes (mw_eof) unless
// ZZ_MEMBERS_NO_EOF is set.
//
// With ZZ_MEMBERS_EXTENDED the level may be 4, 5 or 6: the body is then what the batch call with ZZ_BATCH_EXTENDED writes for the
// block -- the rule above with "levels 0..3" widened, a packet's window being the block's own bytes in front of it. Everything in
// this file sees such a call as level 2 (slots, strides, the stored fallback).
//
// The packet kernels are the batch's (zz_batch.h), with block i as item i. The passes of this file:
//   plan      k_mw_items       per member: srcs[i] = src + i * B, ns[i], first[i] = i * ppm (closed forms: nothing is read back)
//             k_mw_desc        per packet: {member, packet within it, slot offset}
//   sizes     k_mw_sizes       one workgroup: D from the packet offsets, stored = D > S, the member's bytes, their exclusive scan,
//                              the total, fits = total + eof <= cap, the stored count, the caller's offsets array
//   write     k_mw_finalize    one wavefront per member, if fits: header, the CRC-32 fold over its packets, trailer; one lane: EOF
//             k_mw_compact     one wavefront per packet: slot -> its place in the member, for members that are not stored
//             k_mw_stored      l0_encode_packet on the packets of stored members (level 0: of every member), in place
#pragma once
#include "zz_batch.h"

namespace zz {

#define ZZ_MW_HEADER 18
#define ZZ_MW_TRAILER 8
#define ZZ_MW_EOF 28
#define ZZ_MW_MAX_MEMBER 65536u

// a full block's stored member must fit BSIZE's 16 bits
__host__ __device__ inline bool mw_geometry_ok(uint32_t B, uint32_t P)
{
    return B != 0 && B <= ZZ_MW_MAX_MEMBER && P != 0 && ZZ_MW_HEADER + l0_item_bytes(B, P) + ZZ_MW_TRAILER <= ZZ_MW_MAX_MEMBER;
}
__host__ __device__ inline void mw_header(uint32_t member_bytes, uint8_t* out)
{
    const uint8_t h[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
    for (int b = 0; b < 16; ++b) out[b] = h[b];
    out[16] = (uint8_t)(member_bytes - 1);
    out[17] = (uint8_t)((member_bytes - 1) >> 8);
}
// bgzip's empty last member: the header, one empty fixed block (03 00), CRC-32 and ISIZE of nothing
__device__ __forceinline__ void mw_eof(uint8_t* out)
{
    mw_header(ZZ_MW_EOF, out);
    out[18] = 3;
    for (int b = 19; b < ZZ_MW_EOF; ++b) out[b] = 0;
}

struct zz_mw_state {
    uint64_t total;          // the members' bytes
    uint64_t stored;         // members that took the stored fallback
    uint32_t fits;           // total + eof <= cap: the write passes may store
    uint32_t pad;
};

struct zz_mw_params {
    const uint8_t* src; uint64_t n;
    uint8_t* dst; uint64_t cap;
    uint32_t B, P;
    uint32_t members;        // blocks
    uint32_t ppm;            // packets of a full block
    uint32_t eof;            // bytes behind the last member: ZZ_MW_EOF or 0
    int level;
    uint64_t full_slots;     // slot bytes of a full block (levels >= 1)
    // the batch's view of the blocks (filled here, read by the batch forms of the packet kernels)
    const uint8_t** srcs; uint64_t* ns; uint32_t* first; zz_batch_desc* desc;
    // per packet, from the packet kernels and k_scan_sizes
    const uint32_t* sizes; const uint64_t* offsets; const zz_cks* cks; const uint8_t* slots;
    // per member
    uint64_t* moff;          // members + 1 file offsets
    uint8_t* stored;         // took the fallback
    zz_mw_state* st;
    uint64_t* user_offsets;  // the caller's copy of moff, or null
};

__device__ __forceinline__ uint32_t mw_block_bytes(const zz_mw_params& Q, uint32_t i)
{
    const uint64_t left = Q.n - (uint64_t)i * Q.B;
    return left < Q.B ? (uint32_t)left : Q.B;
}

// ---- plan ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mw_items(zz_mw_params Q)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > Q.members) return;
    if (i == Q.members) {                                  // (the entry behind the last member: the call's packets)
        const uint32_t last = Q.members ? mw_block_bytes(Q, Q.members - 1) : 0;
        Q.first[i] = Q.members ? (Q.members - 1) * Q.ppm + (last + Q.P - 1) / Q.P : 0;
        return;
    }
    Q.srcs[i] = Q.src + (uint64_t)i * Q.B;
    Q.ns[i] = mw_block_bytes(Q, i);
    Q.first[i] = i * Q.ppm;
}

__global__ __launch_bounds__(256) void k_mw_desc(zz_mw_params Q, uint32_t npk)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= npk) return;
    zz_batch_desc d;
    d.item = g / Q.ppm;
    d.k = g - d.item * Q.ppm;
    d.slot = (uint64_t)d.item * Q.full_slots + (uint64_t)d.k * zz_slot_stride(Q.level, Q.P);
    Q.desc[g] = d;
}

// ---- sizes --------------------------------------------------------------------------------------------------------------
// One workgroup, four members per thread and round (a round's bytes stay below 2^32: 4096 members of at most 65,536 bytes
// each). A GiB at the default block size is 16,449 members: five rounds.
__global__ __launch_bounds__(ZZ_SCAN_THREADS) void k_mw_sizes(zz_mw_params Q)
{
    __shared__ uint32_t wtot[ZZ_SCAN_THREADS / ZZ_WAVE];
    __shared__ uint32_t nstored;
    const uint32_t t = threadIdx.x;
    if (t == 0) nstored = 0;
    uint64_t carry = 0;
    uint32_t mine_stored = 0;
    for (uint32_t r0 = 0; r0 < Q.members; r0 += 4 * ZZ_SCAN_THREADS) {
        const uint32_t i0 = r0 + 4 * t;
        uint32_t v[4] = { 0, 0, 0, 0 };
        for (uint32_t u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u;
            if (i >= Q.members) break;
            const uint32_t len = mw_block_bytes(Q, i);
            const uint32_t S = (uint32_t)l0_item_bytes(len, Q.P);
            uint32_t body = S;
            bool st = false;
            if (Q.level != 0) {
                const uint32_t f = i * Q.ppm, last = f + (len + Q.P - 1) / Q.P - 1;
                const uint64_t D = Q.offsets[last] + Q.sizes[last] - Q.offsets[f];
                st = D > S;
                if (!st) body = (uint32_t)D;
            }
            Q.stored[i] = st ? 1 : 0;
            mine_stored += st ? 1u : 0u;
            v[u] = ZZ_MW_HEADER + body + ZZ_MW_TRAILER;
        }
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        const wg_prefix<uint32_t> s = wg_scan_excl<ZZ_SCAN_THREADS>(mine, wtot);
        uint64_t o = carry + s.excl;
        for (uint32_t u = 0; u < 4; ++u) {
            if (i0 + u < Q.members) {
                Q.moff[i0 + u] = o;
                if (Q.user_offsets) Q.user_offsets[i0 + u] = o;
            }
            o += v[u];
        }
        carry += s.total;
        __syncthreads();
    }
    if (mine_stored) atomicAdd(&nstored, mine_stored);
    __syncthreads();
    if (t == 0) {
        Q.moff[Q.members] = carry;
        if (Q.user_offsets) Q.user_offsets[Q.members] = carry;
        Q.st->total = carry;
        Q.st->stored = nstored;
        Q.st->fits = carry + Q.eof <= Q.cap ? 1u : 0u;
        Q.st->pad = 0;
    }
}

// ---- write --------------------------------------------------------------------------------------------------------------
// one wavefront per member: what k_batch_finalize does for a gzip item, around a body whose place the scan has decided
#define ZZ_MW_FIN_THREADS 256
__global__ __launch_bounds__(ZZ_MW_FIN_THREADS) void k_mw_finalize(zz_mw_params Q)
{
    if (!Q.st->fits) return;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, per_block = ZZ_MW_FIN_THREADS / ZZ_WAVE;
    const uint32_t xp = gf2_xpow8(Q.P);
    if (blockIdx.x == 0 && threadIdx.x == 0 && Q.eof) mw_eof(Q.dst + Q.st->total);
    for (uint32_t i = blockIdx.x * per_block + wv; i < Q.members; i += gridDim.x * per_block) {
        const uint32_t len = mw_block_bytes(Q, i);
        const uint32_t f = i * Q.ppm, npk = (len + Q.P - 1) / Q.P;
        const uint32_t crc = batch_crc_fold(Q.cks + f, npk, len, Q.P, xp, lane);
        if (lane == 0) {
            const uint64_t at = Q.moff[i];
            const uint32_t bytes = (uint32_t)(Q.moff[i + 1] - at);
            uint8_t* d = Q.dst + at;
            mw_header(bytes, d);
            uint8_t* t = d + bytes - ZZ_MW_TRAILER;
            t[0] = (uint8_t)crc; t[1] = (uint8_t)(crc >> 8); t[2] = (uint8_t)(crc >> 16); t[3] = (uint8_t)(crc >> 24);
            t[4] = (uint8_t)len; t[5] = (uint8_t)(len >> 8); t[6] = (uint8_t)(len >> 16); t[7] = (uint8_t)(len >> 24);
        }
    }
}

// one wavefront per packet: slot -> member, as k_batch_compact
#define ZZ_MW_COMPACT_THREADS 256
__global__ __launch_bounds__(ZZ_MW_COMPACT_THREADS) void k_mw_compact(zz_mw_params Q, uint32_t npk)
{
    if (!Q.st->fits) return;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, per_block = ZZ_MW_COMPACT_THREADS / ZZ_WAVE;
    for (uint32_t g = blockIdx.x * per_block + wv; g < npk; g += gridDim.x * per_block) {
        const zz_batch_desc d = Q.desc[g];
        if (Q.stored[d.item]) continue;
        const uint32_t f = g - d.k;
        coop_copy(Q.dst + Q.moff[d.item] + ZZ_MW_HEADER + (Q.offsets[g] - Q.offsets[f]), Q.slots + d.slot, Q.sizes[g], lane, ZZ_WAVE);
    }
}

// one workgroup per packet of a stored member: its stored blocks straight to their place (no checksum: the CRC-32 partials
// are k_crc32_packets_batch's)
__global__ __launch_bounds__(256) void k_mw_stored(zz_mw_params Q, uint32_t npk)
{
    if (!Q.st->fits) return;
    for (uint32_t g = blockIdx.x; g < npk; g += gridDim.x) {
        const zz_batch_desc d = Q.desc[g];
        if (Q.level != 0 && !Q.stored[d.item]) continue;                              // (uniform: the whole workgroup skips)
        const uint32_t len = mw_block_bytes(Q, d.item);
        zz_packet_params P = {};
        P.src = Q.src + (uint64_t)d.item * Q.B; P.n = len; P.packet_size = Q.P; P.npk = (len + Q.P - 1) / Q.P;
        P.last_is_final = 1; P.cks_kind = ZZ_CKS_NONE;
        uint8_t* at = Q.dst + Q.moff[d.item] + ZZ_MW_HEADER + (uint64_t)d.k * l0_packet_bytes(Q.P, false);
        l0_encode_packet(P, d.k, at, 0, nullptr, nullptr);
    }
}

}  // namespace zz
