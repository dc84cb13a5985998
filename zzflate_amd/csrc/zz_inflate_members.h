// zz_inflate_members.h -- a file of gzip members back to back (zz_decode_members_device, zz_api.hip): RFC 1952 2.2, what
// `cat a.gz b.gz` and bgzip / BAM / tabix (BGZF) write. The rules -- what a member file is, zi_member, zi_members, zi_bc_len,
// the chain check, the hop, the slots and the verdict -- are ZZ_HD functions of zz_inflate_core.h;
// tests/cxx/inflate_members_harness.cpp runs the same procedure with them on the host.
//
// BLOCKED PATH: a member that announces its own length (the extra subfield `BC`) can be cut out without decoding anything, so
// a blocked file is thousands of independent items for k_inflate_items (zz_inflate.h), which decodes them unchanged.
//
//   mark     k_members_mark<false>  every byte offset of the source is tested for a header that announces a length which
//                                   stays inside the file (zi_members_candidate): a bandwidth pass over the compressed bytes,
//                                   16 bytes per lane and load, ZZ_MEM_STRETCH bytes per workgroup, one count per workgroup
//            k_members_scan         exclusive scan of the workgroups' counts (one workgroup); the host reads the total and
//                                   sizes the context's buffers by it -- no constant caps the candidates
//            k_members_mark<true>   the same test again in the workgroups that counted something: the candidates and their
//                                   lengths, written in ascending order (rank inside the workgroup by a scan over its lanes)
//   check    k_members_check        one thread per candidate, one flag: is a link of the chain broken?
//   hop      k_members_hop          only if it is (a member that stores bytes which look like a header): one lane walks the
//                                   chain from offset 0, one dependent load per member, and writes the member list over the
//                                   candidates; a walk that leaves the chain says "not blocked"
//   slots    k_members_slots        ISIZE of every member, its exclusive scan (one workgroup), the descriptors of
//                                   k_inflate_items in the context's buffers, m* and the total
//   decode   k_inflate_items        members 0..m*, launched as zz_decode_batch_device launches it
//   re-judge k_inflate_members      only when m* alone failed, for want of room: from m* on, over what is left of source and
//                                   room -- "no space" from a cut-out member is a claim (zz_inflate_core.h), this is the verdict
//
// The host reads a fixed handful of numbers (zz_mem_state and the two failure counters) whatever the member count.
//
// SERIAL PATH: k_inflate_members, one workgroup of ZZ_INF_THREADS lanes running zi_members -- files whose members carry no
// `BC`, files whose chain cannot be walked, and everything the blocked path hands over because a member failed. It IS the
// definition of the result and runs at ONE wavefront's speed, a few MB/s, like packet_size 0 of zz_decode_device.
//
// Workspace: 12 bytes per ZZ_MEM_STRETCH source bytes and 52 bytes per candidate (its offset and length, and the five descriptor
// arrays, which are sized before the members are known: members <= candidates).
//
// Every kernel reads only [src, src + n) and its workspace and ends for any input: the mark pass reads 18 bytes per lane
// (byte by byte where they would pass the end), zi_bc_len stays inside the bytes it is given, a candidate and a hop's stop
// lie inside the file with their whole length, and a member is at least 22 bytes, so its ISIZE lies inside it.
#pragma once
#include "zz_inflate.h"

namespace zz {

#define ZZ_MEM_THREADS 256
#define ZZ_MEM_PER_LANE 16
#define ZZ_MEM_STRETCH (ZZ_MEM_THREADS * ZZ_MEM_PER_LANE)      // source bytes per workgroup of the mark pass
#define ZZ_MEM_SCAN_THREADS 1024

// what the host reads (all of it written by the device; zeroed, mstar ~0, in front of a call)
struct zz_mem_state {
    unsigned long long candidates;   // k_members_scan
    unsigned long long chain_bad;    // k_members_check: a link of the candidates' chain is broken
    unsigned long long blocked;      // k_members_hop: the member list stands (the candidates, or what the walk found)
    unsigned long long members;      // members of the list
    unsigned long long total;        // k_members_slots: sum of ISIZE
    unsigned long long mstar;        // first member that passes cap (~0: none),
    unsigned long long mstar_src;    //   where it begins in the source
    unsigned long long mstar_dst;    //   and in the destination
};

// offsets [i, i + 16) of the source are this lane's; a header that begins in them may reach into the next lane's or the next
// workgroup's bytes -- it is seen once, by the lane that owns its first byte. Returns the lane's candidates: bit k for offset i + k.
__device__ __forceinline__ uint32_t members_mark_lane(const uint8_t* src, uint64_t n, uint64_t i)
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
    uint32_t hits = 0;                                       // bit k: 1f 8b 08 at i + k
#pragma unroll
    for (uint32_t k = 0; k < ZZ_MEM_PER_LANE; ++k) {
        const uint32_t sh = (k & 3) * 8;
        const uint32_t w = sh ? (d[k >> 2] >> sh) | (d[(k >> 2) + 1] << (32 - sh)) : d[k >> 2];
        hits |= (uint32_t)((w & 0xFFFFFFu) == 0x088B1Fu) << k;
    }
    uint32_t cand = 0;
    for (uint32_t h = hits; h; h &= h - 1) {                 // rare: the rest of the header comes from memory again
        const uint32_t k = (uint32_t)__builtin_ctz(h);
        if (zi_members_candidate(src, n, i + k)) cand |= 1u << k;
    }
    return cand;
}

// FILL = false: blk_cnt[b] = candidates in stretch b. FILL = true: the candidates of stretch b from blk_base[b] on, ascending.
template <bool FILL>
__global__ __launch_bounds__(ZZ_MEM_THREADS) void k_members_mark(const uint8_t* src, uint64_t n, uint32_t* blk_cnt, const uint64_t* blk_base,
                                                                 uint64_t* offs, uint32_t* lens)
{
    __shared__ uint32_t wtot[ZZ_MEM_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (FILL && blk_cnt[b] == 0) return;                     // uniform: most stretches hold no header
    const uint64_t i = b * ZZ_MEM_STRETCH + (uint64_t)t * ZZ_MEM_PER_LANE;
    const uint32_t cand = members_mark_lane(src, n, i);
    const uint32_t mine = (uint32_t)__builtin_popcount(cand);
    const wg_prefix<uint32_t> s = wg_scan_excl<ZZ_MEM_THREADS>(mine, wtot);      // one scan: wtot is not written again
    if (!FILL) { if (t == 0) blk_cnt[b] = s.total; return; }
    uint64_t at = blk_base[b] + s.excl;
    for (uint32_t h = cand; h; h &= h - 1, ++at) {
        const uint32_t k = (uint32_t)__builtin_ctz(h);
        offs[at] = i + k; lens[at] = zi_members_candidate(src, n, i + k);
    }
}

// exclusive scan of the stretches' counts; the total to st->candidates. One workgroup, 4096 counts a round.
__global__ __launch_bounds__(ZZ_MEM_SCAN_THREADS) void k_members_scan(const uint32_t* blk_cnt, uint64_t nblk, uint64_t* blk_base, zz_mem_state* st)
{
    __shared__ uint32_t wtot[ZZ_MEM_SCAN_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t r0 = 0; r0 < nblk; r0 += 4 * ZZ_MEM_SCAN_THREADS) {
        const uint64_t k = r0 + 4 * t;
        uint32_t v[4] = { 0, 0, 0, 0 };
        for (uint32_t u = 0; u < 4; ++u) if (k + u < nblk) v[u] = blk_cnt[k + u];
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];      // at most a third of 4 * ZZ_MEM_STRETCH each: far below 2^32 a round
        const wg_prefix<uint32_t> s = wg_scan_excl<ZZ_MEM_SCAN_THREADS>(mine, wtot);
        uint64_t o = carry + s.excl;
        for (uint32_t u = 0; u < 4; ++u) { if (k + u < nblk) blk_base[k + u] = o; o += v[u]; }
        carry += s.total;
        __syncthreads();
    }
    if (t == 0) st->candidates = carry;
}

// one pass, one flag (every writer stores the same value)
__global__ __launch_bounds__(256) void k_members_check(const uint64_t* offs, const uint32_t* lens, uint64_t m, uint64_t n, zz_mem_state* st)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride)
        if (zi_members_link_broken(j, m, offs[j], lens[j], j + 1 < m ? offs[j + 1] : 0, n)) st->chain_bad = 1ull;
}

// the member list: the candidates when their chain holds, else what one lane's walk finds (written over the candidates, which
// the walk does not read), else none
__global__ void k_members_hop(const uint8_t* src, uint64_t n, uint64_t* offs, uint32_t* lens, uint64_t m, zz_mem_state* st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t members = m;
    if (st->chain_bad) members = zi_members_hop(src, n, offs, lens, m);
    st->members = members;
    st->blocked = members ? 1ull : 0ull;
}

struct zz_mem_slots {
    const uint8_t* src; uint64_t n; uint8_t* dst; uint64_t cap;
    const uint64_t* offs; const uint32_t* lens;
    const uint8_t** srcs; uint64_t* src_lens; uint8_t** dsts; uint64_t* caps;      // k_inflate_items' descriptors
    zz_mem_state* st;
};
// one workgroup, 1024 members a round: ISIZE, its exclusive scan, and the descriptors of the members that are dealt (those
// whose offset lies inside cap: members 0..m*)
__global__ __launch_bounds__(ZZ_MEM_SCAN_THREADS) void k_members_slots(zz_mem_slots Q)
{
    __shared__ uint64_t wtot[ZZ_MEM_SCAN_THREADS / ZZ_WAVE];
    if (!Q.st->blocked) return;                              // uniform
    const uint64_t m = Q.st->members;
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t r0 = 0; r0 < m; r0 += ZZ_MEM_SCAN_THREADS) {
        const uint64_t j = r0 + t;
        uint64_t c = 0; uint32_t len = 0, isize = 0;
        if (j < m) { c = Q.offs[j]; len = Q.lens[j]; isize = zi_members_isize(zi_view<const uint8_t>{ Q.src, Q.n }, c, len); }
        const wg_prefix<uint64_t> s = wg_scan_excl<ZZ_MEM_SCAN_THREADS>((uint64_t)isize, wtot, carry);      // 64 bits: the sum of ISIZE has no bound
        const uint64_t off = s.excl;
        if (j < m && off <= Q.cap) {
            Q.srcs[j] = Q.src + c; Q.src_lens[j] = len;
            Q.dsts[j] = Q.dst + off; Q.caps[j] = zi_members_slot_cap(isize, off, Q.cap);
            // (one member at most gets here and passes cap: those behind m* begin behind cap)
            if (zi_members_is_mstar(isize, off, Q.cap)) { Q.st->mstar = j; Q.st->mstar_src = c; Q.st->mstar_dst = off; }
        }
        carry += s.total;
        __syncthreads();
    }
    if (t == 0) Q.st->total = carry;
}

// the serial path: zi_members over src[0, n) onto dst[0, cap) by one wavefront
struct zz_inf_members_out { int status; uint64_t out; uint64_t members; };
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_members(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap,
                                                                    zz_inf_members_out* res)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    zz_inf_lanes w{ (uint8_t*)ibuf4, lane };
    const zi_members_result R = zi_members(w, src, n, dst, cap, S, lane, ZZ_INF_THREADS);
    if (lane == 0) { res->status = R.status; res->out = R.out; res->members = R.members; }
}

}  // namespace zz
