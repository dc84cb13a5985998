// zz_inflate.h -- decode on the device: parallel inflate of packet-mode streams (zz_decode_device, zz_api.hip).
//
// A packet-mode stream is a run of byte-aligned packets; every non-final one decodes to exactly `packet_size` (P) bytes
// and ends with a one-byte stored block (01 00 FE FF xx), so packet k's output starts at k * P. The work:
//
//   phase 1  k_inflate_packets   one workgroup (one wavefront) per packet: the core of zz_inflate_core.h with the
//                                packet's window in LDS. A byte whose match source lies in front of the packet's start
//                                (levels >= 2 extend matches backward; warm windows and levels 4..6 reach up to 32 KiB
//                                back) is written PENDING: a bit in the packet's bitmap and, in the batch's pointer array,
//                                the absolute position it copies; a copy from a pending byte copies the pointer. No
//                                packet waits for another.
//   phase 2  k_inflate_resolve   rounds of pointer jumping over the packets that hold pending bytes, one launch per
//                                round: a byte whose target was final before the round takes its value, otherwise it
//                                adopts the target's pointer. Targets lie strictly in front, and phase 1 already folded
//                                every chain inside a packet, so a chain has at most one link per packet of the batch:
//                                ceil(log2(packets)) + 1 rounds at most. No workgroup waits for another.
//   discovery k_inflate_scan     candidate packet starts (position + 5 of every 01 00 FE FF) when no index is given;
//                                phase 1 then runs from every candidate and the host keeps the chain of true starts.
//   serial   k_inflate_serial    the same core on one workgroup with the whole output as the window (global memory):
//                                any single-member stream -- the compatibility path.
//   batch    k_inflate_items     many independent streams in one call (zz_decode_batch_device): one wavefront per stream, the
//                                serial path's form of the core (zi_item: container, blocks, trailer and checksum by that one
//                                wavefront), persistent wavefronts dealing themselves the items from a counter. No window in
//                                the LDS, no pending bytes, no phase 2, no index: about 9 KiB of LDS and one wavefront per
//                                workgroup, so sixteen of them are resident on a CU where phase 1 fits three. One item decodes
//                                at ONE wavefront's speed (a few MB/s): a batch is fast when it holds at least as many items
//                                as the GPU holds wavefronts (256 CUs x 16); a stream of hundreds of MiB belongs to
//                                zz_decode_device.
//
// Workspace of one batch of B packets (B * P <= ZZ_INF_BATCH_BYTES, B <= ZZ_INF_BATCH_PACKETS): 4 bytes of pointer per
// output byte, one bit of pending bitmap per output byte and 20 bytes per packet -- at most 264 MiB + 5 MiB, whatever the
// input size; larger calls go through in batches (a batch's pending bytes only point into it or into earlier batches,
// which are final by then). Discovery adds 20 bytes per candidate, at most ZZ_INF_MAX_CANDIDATES of them (80 MiB).
//
// Every kernel reads only [d_src, d_src + src_len) (packet starts and ends are checked against the stream before use),
// writes only [d_dst, d_dst + cap) and its workspace, and ends for any input: every loop is bounded by the input or
// the output it has consumed or produced.
#pragma once
#include "zz_common.h"
#include "zz_wave.h"
#include "zz_inflate_core.h"

namespace zz {

#define ZZ_INF_THREADS 64                       // phase 1 and the serial path: one wavefront
#define ZZ_INF_IBUF 2048                        // LDS bytes of staged input per wavefront
#define ZZ_INF_RES_THREADS 256
#define ZZ_INF_BATCH_BYTES (64ull << 20)        // output bytes per batch (pointers fit ZI_PTR_MASK with ZI_BIAS)
#define ZZ_INF_BATCH_PACKETS (1u << 18)
#define ZZ_INF_MAX_ROUNDS 30                    // the round number lives in the pointer word's top five bits
#define ZZ_INF_MAX_CANDIDATES (1ull << 22)     // discovery: more candidates than this go to the serial path

enum { ZZ_INF_INDEXED = 1, ZZ_INF_DISCOVER = 2 };

// The slots of the counter block `tot` (ZZ_TOT_SLOTS words) that phase 1, phase 2 and the checked reads share with the host
enum { ZZ_TOT_PENDING = 0,        // pending bytes phase 1 left
       ZZ_TOT_OPEN = 1,           // [ZZ_TOT_OPEN + r]: bytes still open after round r (1 .. ZZ_INF_MAX_ROUNDS)
       ZZ_TOT_BAD_SUM = 60,       // checked range read: packets that do not match their checksum (zz_inflate_check.h)
       ZZ_TOT_EXTERNAL = 61,      // range read: bytes of the window that turned external
       ZZ_TOT_UNWRITTEN = 62,     // packets decoded but not written (past cap)
       ZZ_TOT_FAILED = 63,        // packets (points: segments) that do not decode as the index says
       ZZ_TOT_SLOTS = 64 };

// One batch of packets of P bytes, for the host: bitmap words per packet, packets per batch (`most`: no more than the caller
// has), phase 1's dynamic LDS (bitmap, staged input, window); and the rounds that settle any chain over n packets (it has at
// most one link per packet).
struct zz_inf_geom { uint32_t words; uint64_t B; size_t lds; };
inline zz_inf_geom zz_inf_geometry(uint32_t P, uint64_t most)
{
    zz_inf_geom g;
    g.words = ((P + 31) / 32 + 3) & ~3u;
    g.B = ZZ_INF_BATCH_BYTES / P;
    if (g.B > ZZ_INF_BATCH_PACKETS) g.B = ZZ_INF_BATCH_PACKETS;
    if (g.B > most) g.B = most;
    g.lds = (size_t)g.words * 4 + ZZ_INF_IBUF + ((P + 15) & ~15u);
    return g;
}
inline uint32_t zz_inf_rounds(uint64_t n) { uint32_t r = 0; while ((1ull << r) < n) ++r; return r + 2; }

// phase 1: packets [k0, k0 + npk) of the call, `starts` relative to the first DEFLATE byte
struct zz_inf_params {
    const uint8_t* s; uint64_t sn;             // the DEFLATE bytes: [d_src + header, d_src + src_len - trailer)
    const uint64_t* starts; uint64_t nstarts;  // packet starts (indexed: nstarts = packets + 1, the last = sn; discovery: candidates)
    uint64_t k0; uint32_t npk;                 // this batch
    uint64_t npk_total;                        // indexed: packets of the call (the last one carries BFINAL)
    uint32_t P; int mode;
    uint8_t* dst; uint64_t cap;                // a packet whose bytes would not fit [0, cap) is decoded but not written
    uint32_t* st;                              // B * P pointers
    uint32_t* pend;                            // B * words bitmap words
    uint32_t words;                            // bitmap words per packet (multiple of 4)
    uint32_t* pcnt;                            // per packet: pending bytes phase 1 left
    uint32_t* prem;                            // per packet: pending bytes still open (phase 2)
    uint64_t* ends;                            // per packet, at k - ebase: byte behind it (relative to s)
    uint32_t* stat;                            // per packet, at k - ebase: bit 0 ok, bit 1 final, bit 2 not written (past cap),
                                               // bits 3.. bytes produced
    uint64_t ebase;                            // packet number of ends[0] / stat[0] (indexed: the batch's first; discovery: 0)
    unsigned long long* tot;                   // the counter block (ZZ_TOT_*)
};

// the input seen through an LDS stage: bytes g[base, base + ZZ_INF_IBUF) of the run's view g[0, n) (zero outside it)
struct zz_inf_in {
    const uint8_t* g; uint64_t n;
    uint8_t* buf; int64_t base;
    uint32_t lane;
    __device__ __forceinline__ uint64_t peek8(uint64_t pos)
    {
        if ((uint64_t)((int64_t)pos - base) > ZZ_INF_IBUF - 12) {
            // the whole wavefront stages 2 KiB from pos on, 64-byte aligned in memory; bytes outside [0, n) read as zero
            base = (int64_t)pos - (int64_t)(((uintptr_t)(g + pos)) & 63);
            if (base >= 0 && (uint64_t)base + ZZ_INF_IBUF <= n) {
                const uint4* src = (const uint4*)(g + base);
#pragma unroll
                for (uint32_t i = 0; i < ZZ_INF_IBUF / 16 / ZZ_INF_THREADS; ++i)
                    ((uint4*)buf)[lane + i * ZZ_INF_THREADS] = src[lane + i * ZZ_INF_THREADS];
            } else {
                for (uint32_t i = lane; i < ZZ_INF_IBUF; i += ZZ_INF_THREADS) {
                    const int64_t q = base + (int64_t)i;
                    buf[i] = (q >= 0 && (uint64_t)q < n) ? g[q] : (uint8_t)0;
                }
            }
            __syncthreads();
        }
        // three aligned words (an LDS read off four-byte alignment is far slower) and a funnel shift
        const uint32_t off = (uint32_t)((int64_t)pos - base);
        const uint32_t* w = (const uint32_t*)buf + (off >> 2);
        const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
        const uint32_t sh = (off & 3) * 8;
        return sh ? (lo >> sh) | ((uint64_t)w[2] << (64 - sh)) : lo;
    }
};

struct zz_inf_fence { __device__ __forceinline__ void operator()() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); } };
struct zz_inf_or {
    __device__ __forceinline__ void operator()(zi_view<uint32_t>& m, uint64_t q) const { atomicOr(&m.p[q >> 5], 1u << (q & 31)); }
};

__device__ __forceinline__ uint32_t inf_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// dynamic LDS: bitmap words * 4 + ZZ_INF_IBUF + P rounded up to 16
// RANGE (k_inflate_packets_range, zz_decode_range_device): Q.dst is the stage of this batch and holds npk * P bytes, so packet b's
// bytes go to b * P -- where the pointers count from -- and always fit; everything else, `abs` and the checks included, is the same.
// RANGES (form 2, k_inflate_packets_ranges, zz_inflate_ranges.h): the workgroup's packet is what its descriptor says -- stream
// packet d.k of read d.read, whose segment starts at stage packet d.seg0 of the wave; the pointers count from the segment's first
// byte, a failed packet is charged to its read, and ends / stat are kept per stage packet.
struct zz_inf_ranges { const zi_read_desc* desc; zi_read* reads; };
template <int FORM> __device__ __forceinline__ void inflate_packets_body(zz_inf_params Q, zz_inf_ranges X)
{
    constexpr bool RANGE = FORM != 0;
    extern __shared__ uint4 inf_dyn[];
    __shared__ zi_tables S;
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    zi_read_desc D{};
    if (FORM == 2) D = X.desc[b];
    const uint64_t k = FORM == 2 ? D.k : Q.k0 + b;
    uint32_t* pend = (uint32_t*)inf_dyn;
    uint8_t* ibuf = (uint8_t*)inf_dyn + (uint64_t)Q.words * 4;
    uint8_t* win = ibuf + ZZ_INF_IBUF;
    for (uint32_t i = lane; i < Q.words; i += ZZ_INF_THREADS) pend[i] = 0;
    S.kind = 0;
    __syncthreads();

    // where the packet lies; anything the index or the candidates say is checked against the stream first
    uint64_t start = 0, end = 0;
    bool ok = k < Q.nstarts;
    if (ok) {
        start = Q.starts[k];
        if (Q.mode == ZZ_INF_INDEXED) { ok = k + 1 < Q.nstarts; if (ok) end = Q.starts[k + 1]; }
        else end = Q.sn;
        ok = ok && start < end && end <= Q.sn;
    }
    const uint64_t abs = k * (uint64_t)Q.P;
    zi_result R{ ZI_E_DATA, 0, 0, 0 };
    uint32_t np = 0;
    if (ok) {
        zi_view<const uint8_t> view{ Q.s + start, end - start };
        zz_inf_in in{ view.p, view.n, ibuf, -(int64_t)(2 * ZZ_INF_IBUF), lane };
        zi_out_packet<zz_inf_fence, zz_inf_or> o{ zi_view<uint8_t>{ win, Q.P }, zi_view<uint32_t>{ pend, Q.words },
                                                  zi_view<uint32_t>{ Q.st + (uint64_t)b * Q.P, Q.P },
                                                  abs, (int64_t)((uint64_t)(FORM == 2 ? b - D.seg0 : b) * Q.P), 0, 0, false, lane, ZZ_INF_THREADS, {}, {} };
        R = zi_run(in, view, 0, o, S, Q.mode == ZZ_INF_INDEXED ? ZI_RUN_INDEXED : ZI_RUN_DISCOVER, Q.P, lane, ZZ_INF_THREADS);
        np = o.npend;
        if (!R.err && Q.mode == ZZ_INF_INDEXED) {
            const bool last = k + 1 == Q.npk_total;
            if ((R.final != 0) != last || (last && R.end != view.n)) R.err = ZI_E_SHAPE;
        }
    }
    // a packet that decodes but does not fit is not written: the call's result is ZZ_E_NOSPACE if it is a true packet, and
    // discovery can still walk over it if it is not
    const bool fits = !R.err && (RANGE || (abs <= Q.cap && Q.cap - abs >= R.out));
    np = inf_wave_sum(np);
    __syncthreads();
    if (fits) {
        // the window to its place (16-byte stores where the destination allows them)
        uint8_t* d = Q.dst + (RANGE ? (uint64_t)b * Q.P : abs);
        const uint32_t nb = (uint32_t)R.out;
        if ((((uintptr_t)d) & 15) == 0) {
            const uint32_t n16 = nb >> 4;
            for (uint32_t i = lane; i < n16; i += ZZ_INF_THREADS) ((uint4*)d)[i] = ((const uint4*)win)[i];
            for (uint32_t i = (n16 << 4) + lane; i < nb; i += ZZ_INF_THREADS) d[i] = win[i];
        } else {
            for (uint32_t i = lane; i < nb; i += ZZ_INF_THREADS) d[i] = win[i];
        }
        if (np) for (uint32_t i = lane; i < Q.words; i += ZZ_INF_THREADS) Q.pend[(uint64_t)b * Q.words + i] = pend[i];
        if (lane == 0 && np) atomicAdd(&Q.tot[ZZ_TOT_PENDING], (unsigned long long)np);
    }
    // phase 2 looks at a packet only through these: a packet that failed or was not written has nothing pending
    if (lane == 0) { const uint32_t v = fits ? np : 0u; Q.pcnt[b] = v; Q.prem[b] = v; }
    if (FORM == 2) {
        if (lane == 0) {
            Q.ends[b] = R.err ? 0 : start + R.end;
            Q.stat[b] = R.err ? 0u : (1u | (R.final ? 2u : 0u) | ((uint32_t)R.out << 3));
            if (R.err) atomicAdd(&X.reads[D.read].fail, 1u);
        }
    } else if (lane == 0 && k < Q.nstarts) {
        Q.ends[k - Q.ebase] = R.err ? 0 : start + R.end;
        Q.stat[k - Q.ebase] = R.err ? 0u : (1u | (R.final ? 2u : 0u) | (fits ? 0u : 4u) | ((uint32_t)R.out << 3));
        if (R.err) atomicAdd(&Q.tot[ZZ_TOT_FAILED], 1ull);
        else if (!fits) atomicAdd(&Q.tot[ZZ_TOT_UNWRITTEN], 1ull);
    }
}
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_packets(zz_inf_params Q) { inflate_packets_body<0>(Q, zz_inf_ranges{ nullptr, nullptr }); }
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_packets_range(zz_inf_params Q) { inflate_packets_body<1>(Q, zz_inf_ranges{ nullptr, nullptr }); }
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_packets_ranges(zz_inf_params Q, zz_inf_ranges X) { inflate_packets_body<2>(Q, X); }

// phase 2, round `round` (1-based) over the batch [k0, k0 + npk); `base` = absolute output position of its first byte
struct zz_res_params {
    uint8_t* dst; uint64_t base; uint32_t P, npk, words;
    uint32_t* st; const uint32_t* pend; const uint32_t* pcnt; uint32_t* prem;
    unsigned long long* tot;
};
// what the range form (k_inflate_resolve_range) knows on top: dst is the stage -- ZI_BIAS carried bytes of the batch before, then
// this batch's -- and base = ZI_BIAS, so a target below the batch base reads a carried byte; `carry` has one bit per carried
// byte: external (zz_inflate_core.h). Bytes that turn external inside [wlo, whi) (relative to the batch base) are counted in tot[ZZ_TOT_EXTERNAL].
struct zz_res_range { const uint32_t* carry; int64_t wlo, whi; };
// RANGES (form 2, k_inflate_resolve_ranges): the stage holds a wave of segments and base = 0; a pointer counts from its segment's
// first byte, stage packet d.seg0, and a target below that is external -- nothing is carried, segments do not span batches. The
// external bytes inside the read's window (bytes [d.lo, d.hi) of this packet) are counted in the read's record.
template <int FORM> __device__ __forceinline__ void inflate_resolve_body(zz_res_params Q, zz_res_range X, zz_inf_ranges Z, uint32_t round)
{
    constexpr bool RANGE = FORM != 0;
    __shared__ uint32_t red[ZZ_INF_RES_THREADS / ZZ_WAVE];
    const uint32_t k = blockIdx.x;
    if (Q.pcnt[k] == 0 || Q.prem[k] == 0) return;         // uniform per workgroup
    const uint32_t t = threadIdx.x;
    uint32_t left = 0, nx = 0;
    zi_read_desc D{};
    if (FORM == 2) D = Z.desc[k];
    const uint64_t sb = FORM == 2 ? (uint64_t)D.seg0 * Q.P : 0;          // where the pointers of this packet count from
    for (uint32_t q = t; q < Q.P; q += ZZ_INF_RES_THREADS) {
        if (!((Q.pend[(uint64_t)k * Q.words + (q >> 5)] >> (q & 31)) & 1u)) continue;
        const uint64_t x = (uint64_t)k * Q.P + q;
        const uint32_t s = Q.st[x];
        if (s >> 27) continue;                            // final (or external) since an earlier round
        const int64_t y = (int64_t)(s & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
        bool fin = y < 0;                                 // an earlier batch: final (phase 1 refused anything in front of the stream)
        bool ext = false;
        if (FORM == 1 && fin) { ext = zi_range_external(y, zi_view<const uint32_t>{ X.carry, ZI_BIAS / 32 }); fin = !ext; }
        if (FORM == 2 && fin) { ext = true; fin = false; }
        if (y >= 0) {
            const uint64_t ky = (sb + (uint64_t)y) / Q.P, qy = (uint64_t)y % Q.P;
            fin = Q.pcnt[ky] == 0 || !((Q.pend[ky * Q.words + (qy >> 5)] >> (qy & 31)) & 1u);
            if (!fin) {
                const uint32_t sy = Q.st[sb + y];
                const uint32_t ry = sy >> 27;
                if (RANGE && ry == ZI_ROUND_EXTERNAL) ext = true;   // it stays external, whenever the target was marked
                else if (ry != 0 && ry < round) fin = true; // final before this round began: its byte is in place
                else { Q.st[x] = sy & ZI_PTR_MASK; ++left; } // adopt its pointer (the old one or this round's: both lead there)
            }
        }
        if (fin) {
            Q.dst[Q.base + x] = Q.dst[(int64_t)(Q.base + sb) + y];
            Q.st[x] = (s & ZI_PTR_MASK) | (round << 27);
        }
        if (RANGE && ext) {
            Q.st[x] = (s & ZI_PTR_MASK) | (ZI_ROUND_EXTERNAL << 27);
            if (FORM == 2 ? (q >= D.lo && q < D.hi) : ((int64_t)x >= X.wlo && (int64_t)x < X.whi)) ++nx;
        }
    }
    if (RANGE) {
        nx = inf_wave_sum(nx);
        if (FORM == 2) { if ((t & 63) == 0 && nx) atomicAdd(&Z.reads[D.read].ext, nx); }
        else if ((t & 63) == 0 && nx) atomicAdd(&Q.tot[ZZ_TOT_EXTERNAL], (unsigned long long)nx);
    }
    left = inf_wave_sum(left);
    if ((t & 63) == 0) red[t >> 6] = left;
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < ZZ_INF_RES_THREADS / ZZ_WAVE; ++w) sum += red[w];
        Q.prem[k] = sum;
        if (sum) atomicAdd(&Q.tot[ZZ_TOT_OPEN + round], (unsigned long long)sum);
    }
}
__global__ __launch_bounds__(ZZ_INF_RES_THREADS) void k_inflate_resolve(zz_res_params Q, uint32_t round)
{
    inflate_resolve_body<0>(Q, zz_res_range{ nullptr, 0, 0 }, zz_inf_ranges{ nullptr, nullptr }, round);
}
__global__ __launch_bounds__(ZZ_INF_RES_THREADS) void k_inflate_resolve_range(zz_res_params Q, zz_res_range X, uint32_t round)
{
    inflate_resolve_body<1>(Q, X, zz_inf_ranges{ nullptr, nullptr }, round);
}
__global__ __launch_bounds__(ZZ_INF_RES_THREADS) void k_inflate_resolve_ranges(zz_res_params Q, zz_inf_ranges Z, uint32_t round)
{
    inflate_resolve_body<2>(Q, zz_res_range{ nullptr, 0, 0 }, Z, round);
}

// range decode, between two batches: the last ZI_BIAS bytes of the finished batch (stage[ZI_BIAS + n - ZI_BIAS + i]) move to the
// front of the stage, and next[i / 32] says which of them are external. One thread per byte: ZI_BIAS / 256 workgroups of 256.
// n >= ZI_BIAS is the caller's (a batch that is not the last is full): the bytes read and the bytes written do not overlap.
// `next` may be the bitmap the batch's rounds read: nothing here reads it.
__global__ __launch_bounds__(256) void k_inflate_range_carry(uint8_t* stage, uint64_t n, uint32_t P, uint32_t words, const uint32_t* st,
                                                             const uint32_t* pend, const uint32_t* pcnt, uint32_t* next)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;       // < ZI_BIAS
    const uint64_t x = n - ZI_BIAS + i;
    stage[i] = stage[(uint64_t)ZI_BIAS + x];
    const uint64_t k = x / P; const uint32_t q = (uint32_t)(x % P);
    const bool ext = pcnt[k] != 0 && ((pend[k * words + (q >> 5)] >> (q & 31)) & 1u) && (st[x] >> 27) == ZI_ROUND_EXTERNAL;
    const unsigned long long m = __ballot(ext);
    if ((threadIdx.x & 63) == 0) { next[i >> 5] = (uint32_t)m; next[(i >> 5) + 1] = (uint32_t)(m >> 32); }
}

// range decode: n bytes from the stage to the caller's destination; 16-byte stores once the destination is aligned (the source
// is read as it lies). Grid-stride, any launch shape.
__global__ __launch_bounds__(256) void k_inflate_range_copy(const uint8_t* src, uint8_t* dst, uint64_t n)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (uint64_t)gridDim.x * blockDim.x;
    uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    const uint64_t n16 = (n - head) >> 4;
    if (t < head) dst[t] = src[t];
    for (uint64_t i = t; i < n16; i += nt) {
        uint4 v;
        __builtin_memcpy(&v, src + head + (i << 4), 16);
        *(uint4*)(dst + head + (i << 4)) = v;
    }
    const uint64_t done = head + (n16 << 4);
    if (t < n - done) dst[done + t] = src[done + t];
}

// discovery: every `01 00 FE FF` in s[0, sn) gives the candidate start i + 5 (if that is inside the stream). The
// candidates are appended in any order (the host sorts them); count may exceed cap, then only the count is meaningful.
__global__ void k_inflate_scan(const uint8_t* s, uint64_t sn, uint64_t* cand, unsigned long long* count, uint64_t cap)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 5 < sn; i += stride) {
        if (s[i] != 0x01 || s[i + 1] != 0x00 || s[i + 2] != 0xFE || s[i + 3] != 0xFF) continue;
        const unsigned long long j = atomicAdd(count, 1ull);
        if (j < cap) cand[j] = i + 5;
    }
}

// the serial path: view = s[0, sn) (DEFLATE bytes and trailer), output d_dst[0, cap)
struct zz_inf_serial_out { int err; int final; uint64_t end; uint64_t out; };
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_serial(const uint8_t* s, uint64_t sn, uint8_t* dst, uint64_t cap,
                                                                   zz_inf_serial_out* res)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    S.kind = 0;
    __syncthreads();
    zi_view<const uint8_t> view{ s, sn };
    zz_inf_in in{ s, sn, (uint8_t*)ibuf4, -(int64_t)(2 * ZZ_INF_IBUF), lane };
    zi_out_linear<zz_inf_fence> o{ zi_view<uint8_t>{ dst, cap }, 0, lane, ZZ_INF_THREADS, {} };
    const zi_result R = zi_run(in, view, 0, o, S, ZI_RUN_STREAM, 0, lane, ZZ_INF_THREADS);
    if (lane == 0) { res->err = R.err; res->final = R.final; res->end = R.end; res->out = R.out; }
}

// ---- a batch of independent streams: one wavefront per item (zz_decode_batch_device) ------------------------------------
#define ZZ_INF_ITEM_WG_PER_CU 16                // resident workgroups (= wavefronts) per CU the grid is sized for
struct zz_inf_items_params {
    const uint8_t* const* srcs; const uint64_t* src_lens;
    uint8_t* const* dsts; const uint64_t* caps;
    uint64_t* out_lens; int32_t* status;       // status may be null
    uint32_t nitems; int format;
    unsigned int* next;                         // the next item to deal out (zero on entry)
    unsigned long long* fails;                  // [0] items with ZZ_E_DATA / ZZ_E_UNSUPPORTED, [1] items with ZZ_E_NOSPACE
};
// zi_item's lane group: one wavefront, the input through the LDS stage, sums by cross-lane shuffles
struct zz_inf_lanes {
    typedef zz_inf_in in_t;
    typedef zz_inf_fence fence_t;
    uint8_t* ibuf; uint32_t lane;
    __device__ __forceinline__ in_t input(const uint8_t* p, uint64_t n) const { return in_t{ p, n, ibuf, -(int64_t)(2 * ZZ_INF_IBUF), lane }; }
    __device__ __forceinline__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
    __device__ __forceinline__ uint64_t sum(uint64_t v) const { return wave_sum64(v); }
    __device__ __forceinline__ uint32_t fold_xor(uint32_t v) const
    {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v ^= __shfl_xor(v, o);
        return v;
    }
};
__global__ __launch_bounds__(ZZ_INF_THREADS) void k_inflate_items(zz_inf_items_params Q)
{
    __shared__ zi_tables S;
    __shared__ uint4 ibuf4[ZZ_INF_IBUF / 16];
    const uint32_t lane = threadIdx.x;
    zz_inf_lanes w{ (uint8_t*)ibuf4, lane };
    for (;;) {
        // lane 0 draws the item, every lane gets its number
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(Q.next, 1u);
        i = uniform(i);
        if (i >= Q.nitems) break;
        const zi_item_result r = zi_item(w, Q.srcs[i], Q.src_lens[i], Q.dsts[i], Q.caps[i], Q.format, S, lane, ZZ_INF_THREADS);
        if (lane == 0) {
            Q.out_lens[i] = r.status == ZI_ITEM_OK ? r.out : ~0ull;
            if (Q.status) Q.status[i] = r.status;
            if (r.status == ZI_ITEM_NOSPACE) atomicAdd(&Q.fails[1], 1ull);
            else if (r.status != ZI_ITEM_OK) atomicAdd(&Q.fails[0], 1ull);
        }
        __syncthreads();                        // the next item's first stage overwrites the input buffer
    }
}

// the trailer against the checksum of the decoded bytes (zz_checksum.h's partials, folded by k_cks_reduce)
__global__ void k_inflate_trailer(const uint8_t* t, int format, const zz_cks_total* cks, uint64_t n, uint32_t* ok)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool good = true;
    if (format == ZZ_FMT_ZLIB) {
        const uint32_t want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
        const uint32_t part = n ? (((uint32_t)cks->b << 16) | cks->a) : 0u;
        good = adler_combine(1u, part, n) == want;
    } else if (format == ZZ_FMT_GZIP) {
        const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        good = (n ? cks->a : 0u) == c && l == (uint32_t)n;
    }
    *ok = good ? 1u : 0u;
}

}  // namespace zz
