// zz_inflate_ranges.h -- many reads of one indexed stream in one call (zz_decode_ranges_device, zz_api.hip): the kernels beside
// zz_inflate.h's third forms of phase 1 and the rounds (k_inflate_packets_ranges, k_inflate_resolve_ranges). The rules -- which
// packets a read needs, its look-back and growth, what a wave is, the verdict -- are ZZ_HD functions of zz_inflate_core.h;
// tests/cxx/inflate_ranges_harness.cpp runs the same procedure with them on the host.
//
//   plan     k_ranges_plan     once per attempt, one workgroup: per unfinished read its segment [k0 - h, k1) and, by an exclusive
//                              scan over the reads, the segment's first stage packet; ZZ_E_ARG, empty and too-long reads are
//                              settled here. Segment r belongs to wave floor(base_r / W), W = one batch of packets; per wave the
//                              first stage packet and the first read (atomic minima). Reads whose wave would lie past
//                              ZZ_RNG_MAX_WAVES wait for the next attempt with their look-back unchanged.
//   per wave k_ranges_desc     one thread per stage packet: its read (binary search over the reads' bases) and its descriptor
//            phase 1, rounds   zz_inflate.h, ceil(log2(longest segment)) + 2 rounds
//            (checked calls)   zz_inflate_check.h: the wave's touched packets summed on the stage and held to the sidecar; a mismatch is
//                              charged to the packet's read as a failed packet, in front of the verdict
//            k_ranges_verdict  one thread per read of the wave: zi_ranges_verdict; status and out_len of a settled read
//            k_ranges_copy     one workgroup per stage packet: its share of the window to d_dsts[read], for reads settled ZZ_OK
//
// The host reads one zz_rng_totals (nine words and the wave table) per attempt, whatever the number of reads.
//
// Workspace. A wave holds fewer than W + (longest segment) <= 2 * W stage packets, W * P <= ZZ_INF_BATCH_BYTES: at most twice
// zz_decode_range_device's -- per stage packet P bytes of stage, 4 * P of pointers, the bitmap words and 20 bytes, plus 24 bytes
// of descriptor -- that is at most 2 * (64 + 256 + 8 + 5) MiB + 12 MiB, and 48 bytes per read. The buffers are sized by the
// largest wave of the call, not by this bound.
#pragma once
#include "zz_inflate.h"

namespace zz {

#define ZZ_RNG_MAX_WAVES 1024u
#define ZZ_RNG_PLAN_PER 4
#define ZZ_RNG_PLAN_THREADS 1024

// what the host reads per attempt (all of it written by the device)
struct zz_rng_totals {
    unsigned long long nwaves;        // waves of this attempt
    unsigned long long stage_end;     // stage packets of this attempt (the end of its last wave)
    unsigned long long longest;       // packets of its longest segment
    unsigned long long deferred;      // reads left to a later attempt because the wave table was full
    unsigned long long n_data, n_unsupported, n_arg, n_nospace;     // reads settled with these, over the whole call
    unsigned long long retried;       // reads that needed more than one attempt, over the whole call
    unsigned long long wave_first[ZZ_RNG_MAX_WAVES + 1];            // first stage packet of wave w (~0: no such wave)
    unsigned long long wave_read[ZZ_RNG_MAX_WAVES + 1];             // first read of wave w
};

struct zz_rng_params {
    const uint64_t* firsts; const uint64_t* nbytes; uint8_t* const* dsts; const uint64_t* caps;
    uint64_t* out_lens; int32_t* status;       // status may be null
    uint64_t nranges; uint64_t npk; uint32_t P;
    uint64_t limit;                            // packets a segment may hold
    uint64_t W;                                // wave capacity in stage packets
    zi_read* reads; zz_rng_totals* tot;
    const uint32_t* cks; uint64_t total_len;   // a checked call's sidecar and decoded length (zz_inflate_check.h); null: unchecked
};

__device__ __forceinline__ void ranges_settle(const zz_rng_params& Q, uint64_t r, const zi_read& R)
{
    Q.out_lens[r] = R.status == ZI_RV_OK ? R.m : ~0ull;
    if (Q.status) Q.status[r] = R.status;
    if (R.status == ZI_RV_DATA) atomicAdd(&Q.tot->n_data, 1ull);
    else if (R.status == ZI_RV_UNSUPPORTED) atomicAdd(&Q.tot->n_unsupported, 1ull);
    else if (R.status == ZI_RV_ARG) atomicAdd(&Q.tot->n_arg, 1ull);
    else if (R.status == ZI_RV_NOSPACE) atomicAdd(&Q.tot->n_nospace, 1ull);
}

// the call's first plan has `fresh` set: the records are made here (no pass over the reads in front of it)
__global__ __launch_bounds__(ZZ_RNG_PLAN_THREADS) void k_ranges_plan(zz_rng_params Q, int fresh)
{
    __shared__ uint64_t wsum[ZZ_RNG_PLAN_THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i <= ZZ_RNG_MAX_WAVES; i += ZZ_RNG_PLAN_THREADS) { Q.tot->wave_first[i] = ~0ull; Q.tot->wave_read[i] = ~0ull; }
    if (t == 0) {
        Q.tot->nwaves = 0; Q.tot->stage_end = 0; Q.tot->longest = 0; Q.tot->deferred = 0;
        if (fresh) { Q.tot->n_data = 0; Q.tot->n_unsupported = 0; Q.tot->n_arg = 0; Q.tot->n_nospace = 0; Q.tot->retried = 0; }
    }
    __syncthreads();
    uint64_t carry = 0;
    for (uint64_t r0 = 0; r0 < Q.nranges; r0 += (uint64_t)ZZ_RNG_PLAN_PER * ZZ_RNG_PLAN_THREADS) {
        const uint64_t i0 = r0 + (uint64_t)t * ZZ_RNG_PLAN_PER;
        uint64_t len[ZZ_RNG_PLAN_PER], mine = 0;
#pragma unroll
        for (int u = 0; u < ZZ_RNG_PLAN_PER; ++u) {
            len[u] = 0;
            const uint64_t r = i0 + u;
            if (r >= Q.nranges) continue;
            zi_read R;
            if (fresh) R = zi_read{ 0, 0, 0, 0, ZI_RS_NEW, 0, 0, 0, 0 };
            else R = Q.reads[r];
            const bool open = R.state != ZI_RS_DONE;
            len[u] = zi_ranges_plan(R, Q.firsts[r], Q.nbytes[r], Q.P, Q.npk, Q.limit);
            R.npk = (uint32_t)len[u];
            Q.reads[r] = R;
            if (open && R.state == ZI_RS_DONE) ranges_settle(Q, r, R);
            mine += len[u];
        }
        const wg_prefix<uint64_t> s = wg_scan_excl<ZZ_RNG_PLAN_THREADS>(mine, wsum, carry);      // segment lengths: the first stage packet
        uint64_t base = s.excl;
#pragma unroll
        for (int u = 0; u < ZZ_RNG_PLAN_PER; ++u) {
            const uint64_t r = i0 + u;
            if (r < Q.nranges) {
                const uint64_t w = zi_ranges_wave(base, Q.W);
                if (len[u] && w >= ZZ_RNG_MAX_WAVES) {   // a later attempt's: bases are ascending, so these are the call's last reads
                    Q.reads[r].npk = 0;
                    atomicAdd(&Q.tot->deferred, 1ull);
                } else if (len[u]) {
                    atomicMin(&Q.tot->wave_first[w], (unsigned long long)base);
                    atomicMin(&Q.tot->wave_read[w], (unsigned long long)r);
                    atomicMax(&Q.tot->nwaves, (unsigned long long)(w + 1));
                    atomicMax(&Q.tot->stage_end, (unsigned long long)(base + len[u]));
                    atomicMax(&Q.tot->longest, (unsigned long long)len[u]);
                }
                Q.reads[r].base = base;
            }
            base += len[u];
        }
        carry += s.total;
        __syncthreads();
    }
}

// stage packets [g0, g0 + n) of the attempt are this wave's; its reads lie in [rlo, rhi). The read of stage packet g is the last one
// whose base is at or below g (reads without a segment share their successor's base and are skipped by the search).
__global__ __launch_bounds__(256) void k_ranges_desc(zz_rng_params Q, uint64_t g0, uint32_t n, uint64_t rlo, uint64_t rhi, zi_read_desc* desc)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t g = g0 + j;
    uint64_t lo = rlo, hi = rhi;                           // base[lo] <= g < base[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (Q.reads[mid].base <= g) lo = mid;
        else hi = mid;
    }
    const zi_read R = Q.reads[lo];
    desc[j] = zi_ranges_desc(R, (uint32_t)lo, g - R.base, (uint32_t)(R.base - g0), Q.firsts[lo], Q.nbytes[lo], Q.P, Q.cks != nullptr);
}

// one thread per read of the wave; `stat` is phase 1's, per stage packet of the wave
__global__ __launch_bounds__(256) void k_ranges_verdict(zz_rng_params Q, uint64_t g0, uint64_t rlo, uint64_t rhi, const uint32_t* stat)
{
    const uint64_t r = rlo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rhi) return;
    zi_read R = Q.reads[r];
    if (R.npk == 0) return;                                // settled before, or deferred
    const uint32_t last_out = stat[R.base - g0 + R.npk - 1] >> 3;
    const uint32_t before = R.tries;
    const int v = zi_ranges_verdict(R, Q.firsts[r], Q.nbytes[r], Q.caps[r], Q.P, Q.npk, Q.limit, last_out);
    if (v == ZI_RV_AGAIN && before == 0) atomicAdd(&Q.tot->retried, 1ull);
    Q.reads[r] = R;
    if (v != ZI_RV_AGAIN) ranges_settle(Q, r, R);
}

// one workgroup per stage packet: bytes [lo, hi) of it, cut at the read's m, to the read's destination. 16-byte stores once the
// destination is aligned (the source is read as it lies). The cut is made here from the read itself: a checked call's descriptors
// hold the widened window.
__global__ __launch_bounds__(256) void k_ranges_copy(zz_rng_params Q, const zi_read_desc* desc, const uint8_t* stage)
{
    const zi_read_desc D = desc[blockIdx.x];
    const zi_read R = Q.reads[D.read];
    if (R.state != ZI_RS_DONE || R.status != ZI_RV_OK) return;          // unfinished or failed: nothing is copied in this attempt
    const uint64_t first = Q.firsts[D.read];
    uint32_t lo, hi;
    zi_ranges_cut(D.k, first, Q.nbytes[D.read], Q.P, &lo, &hi);
    const uint64_t a = D.k * Q.P + lo;                      // stream position of the first byte to copy: >= first
    uint64_t e = D.k * Q.P + hi;
    if (e > first + R.m) e = first + R.m;
    if (e <= a) return;
    const uint64_t n = e - a;
    const uint8_t* src = stage + (uint64_t)blockIdx.x * Q.P + lo;
    uint8_t* dst = Q.dsts[D.read] + (a - first);
    const uint32_t t = threadIdx.x;
    uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    const uint64_t n16 = (n - head) >> 4;
    if (t < head) dst[t] = src[t];
    for (uint64_t i = t; i < n16; i += 256) {
        uint4 v;
        __builtin_memcpy(&v, src + head + (i << 4), 16);
        *(uint4*)(dst + head + (i << 4)) = v;
    }
    const uint64_t done = head + (n16 << 4);
    if (t < n - done) dst[done + t] = src[done + t];
}

// a failure of the call itself: every read gets its code
__global__ __launch_bounds__(256) void k_ranges_fill(uint64_t* out_lens, int32_t* status, uint64_t nranges, int32_t code)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nranges; r += stride) {
        out_lens[r] = ~0ull;
        if (status) status[r] = code;
    }
}

}  // namespace zz
