// zz_common.h -- shared constants and launch-parameter structs for the MI355X DEFLATE encoder.
//
// Vocabulary follows the reference (jandevaan/zzflate): a *packet* is one independently encoded input
// range (the lambda at zzflate.cpp:101-125); its output is a byte-aligned run of complete DEFLATE blocks,
// so packet outputs concatenate by plain byte copy (zzflate.cpp:134-155). One packet = one wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZZ_WAVE 64
#define ZZ_HASH_BITS 13                 // encoder.h:41
#define ZZ_HASH_SIZE (1 << ZZ_HASH_BITS)
#define ZZ_MAX_LEN 258                  // encoder.h:47
#define ZZ_MAX_PACKET 32768             // positions fit 15 bits -> u16 table entries (pos+1, 0 = empty)
#define ZZ_BATCH_LEN 16384              // encoder.cpp:227

enum { ZZ_FMT_ZLIB = 0, ZZ_FMT_GZIP = 1, ZZ_FMT_DEFLATE = 2 };   // zzflate.h:8
enum { ZZ_CKS_NONE = 0, ZZ_CKS_ADLER = 1, ZZ_CKS_CRC = 2 };

// Per-packet checksum partial. Adler: (a, b) of the packet computed with start value 0
// (adler.cpp:5-15 `combine` semantics). CRC: a = crc32 of the packet with start value 0, b unused.
struct zz_cks { uint32_t a, b; };

struct zz_packet_params {
    const uint8_t* src;       // first byte of this shard
    uint64_t n;               // shard length in bytes
    uint64_t halo;            // readable bytes in front of src (level >= 2 backward extension, encoder.cpp:404)
    uint32_t packet_size;     // bytes per packet (last one may be shorter)
    uint32_t npk;             // number of packets in the shard
    int last_is_final;        // last packet of the shard carries BFINAL
    int cks_kind;             // ZZ_CKS_*
    uint8_t* slots;           // npk worst-case sized output slots
    uint32_t slot_stride;     // bytes per slot (multiple of 16)
    uint32_t* sizes;          // out: bytes written per packet
    zz_cks* cks;              // out: checksum partial per packet (may be null when cks_kind == NONE)
    uint32_t* err;            // out: sticky error word (slot overflow etc.)
    unsigned long long* prof; // diagnostic builds (-DZZ_PROF) only: per-phase cycle sums; ignored otherwise
    uint32_t warm;            // level 1: bytes in front of a packet hashed into its table before the parse (0: cold, the reference)
    const uint8_t* tail;      // k_encode_l1p: 128 bytes, the shard's last min(n, 64) bytes followed by zeros (k_fill_tail)
    uint32_t dbg_viol;        // tests: report the LDS-order check as failed (error bit 4) whatever it saw
};
// bits of *err
#define ZZ_ERR_SLOT_OVERFLOW 1u
#define ZZ_ERR_LDS_ORDER 4u   // a kernel saw a slot keep a LOWER lane's store of an instruction a higher lane took part in

// worst-case bytes one packet of `len` input bytes can occupy in its slot, per level (multiple of 16)
__host__ __device__ inline uint32_t zz_slot_stride(int level, uint32_t len)
{
    uint64_t b;
    if (level == 0) b = (uint64_t)len + 10;
    else if (level == 1) b = ((uint64_t)9 * len + 10 + 7) / 8 + 6;   // 3 + 9 bits/byte + EOB, + 1-byte stored block
    else b = (uint64_t)len + 11;                                      // stored fallback is the worst case
    b += 8;                                                           // the ring stores whole words
    return (uint32_t)((b + 15) & ~15ull);
}

// ---- batches (zz_encode_batch_device, zz_batch.h) ----------------------------------------------------------------
// Many independent items in one launch. Packets are numbered across the batch (item 0's first, then item 1's, ...); a
// packet's descriptor says whose it is. Each item is a stream of its own: cold packets, its own end, its own tail.
struct zz_batch_desc {
    uint32_t item;            // the item the packet belongs to
    uint32_t k;               // its index within the item
    uint64_t slot;            // byte offset of its slot in the batch's slots (slots are sized by the packet's own length)
};
struct zz_batch_map {
    const zz_batch_desc* desc;      // one per packet of the batch
    const uint8_t* const* srcs;     // per item: first input byte
    const uint64_t* ns;             // per item: input bytes
    const uint32_t* first;          // per item + 1: the item's first packet (exclusive scan of the packet counts)
    const uint8_t* tails;           // per item: 128 bytes, its last min(n, 64) bytes followed by zeros (k_fill_tail)
    uint32_t npk;                   // packets of the batch
    int level;                      // slot strides: zz_slot_stride(level, len)
};
struct zz_no_batch {};              // the single-stream forms: the packet index is the shard's own

// The packet-kernel bodies see a packet through zz_packet_params P and its index k in P's shard. A single stream's is the
// launch's own P with k = g. A batch packet g gets a P of its own, built from its descriptor: the item as the shard (its
// src, n and tail, no halo, the last packet final), and sizes / cks / slots based so that index k lands on packet g's
// entries and slot. The slot stride is the packet's own (zz_slot_stride of its length), so the overflow check is exact.
__device__ __forceinline__ uint32_t zz_batch_npk(const zz_packet_params& P, const zz_no_batch&) { return P.npk; }
__device__ __forceinline__ uint32_t zz_batch_npk(const zz_packet_params&, const zz_batch_map& M) { return M.npk; }
__device__ __forceinline__ const zz_packet_params& zz_packet_view(const zz_packet_params& P, const zz_no_batch&, uint32_t g, uint32_t& k)
{
    k = g;
    return P;
}
__device__ __forceinline__ zz_packet_params zz_packet_view(const zz_packet_params& B, const zz_batch_map& M, uint32_t g, uint32_t& k)
{
    const zz_batch_desc d = M.desc[g];
    zz_packet_params P = B;
    const uint32_t f = g - d.k;                       // the item's first packet
    k = d.k;
    P.src = M.srcs[d.item];
    P.n = M.ns[d.item];
    P.halo = 0;                                       // nothing in front of an item belongs to its stream
    P.npk = M.first[d.item + 1] - f;
    P.last_is_final = 1;
    P.tail = M.tails + (uint64_t)d.item * 128;
    const uint32_t len = k + 1 < P.npk ? P.packet_size : (uint32_t)(P.n - (uint64_t)k * P.packet_size);
    P.slot_stride = zz_slot_stride(M.level, len);
    P.slots = B.slots + d.slot - (uint64_t)k * P.slot_stride;    // P.slots + k * P.slot_stride = this packet's slot
    P.sizes = B.sizes + f;
    P.cks = B.cks + f;
    return P;
}

// ---- the sequential stream's output buffers (outputbitstream.h:171-201) ------------------------------------------
// A single Encoder asks EnsureOutputLength(length) at every block start. With a caller-owned buffer the answer is the
// room left in it; through the callback API the library owns chunks of 1,000,000 bytes and opens a new one when the
// current one is not "enough" (more than twice the length asked for, or more than 2^18 bytes). Block sizes at level 1
// follow from that answer (encoder.cpp:331-337), and the chunks are what the callback receives (zzflate.cpp:207-215),
// so the rule is shared by the stream kernels (which apply it) and the host (which replays the kernels' log of
// (bytes stored, length asked for) pairs to find the chunk boundaries).
#define ZZ_CHUNK_BYTES 1000000ll
struct zz_chunker {
    uint64_t chunk_start;     // bytes stored when the current chunk was opened
    uint32_t nchunks;         // chunks opened so far
};
// returns AvailableBytes() after the call; *opened = a new chunk starts at `stored`
__host__ __device__ inline int64_t zz_chunk_ensure(zz_chunker& k, uint64_t stored, int64_t length, bool* opened)
{
    const int64_t avail = k.nchunks ? (int64_t)(k.chunk_start + ZZ_CHUNK_BYTES) - (int64_t)stored : 0;
    *opened = false;
    if (avail > 2 * length || avail > (1 << 18)) return avail;          // IsEnough, outputbitstream.h:192-201
    k.chunk_start = stored;
    k.nchunks++;
    *opened = true;
    return ZZ_CHUNK_BYTES;
}
// what the stream kernels get besides zz_packet_params
struct zz_stream_ctl {
    uint64_t cap;             // fixed form: bytes of the caller's buffer behind the container header (encoder sees dest+hl)
    int chunked;              // 0: caller-owned buffer of `cap` bytes, 1: library-owned chunks (callback API)
    uint64_t* log;            // chunked: (bytes stored, length asked for) per EnsureOutputLength call, or null
    uint32_t log_cap;         // pairs that fit
    uint32_t* log_n;          // pairs written (may exceed log_cap: the host then reports an error)
    uint32_t* truncated;      // set when the reference would have stopped early (no room left): the stream is incomplete
};
__device__ __forceinline__ void zz_log_ensure(const zz_stream_ctl& C, uint32_t& nlog, uint64_t stored, uint64_t need)
{
    if ((threadIdx.x & 63) == 0 && C.log && nlog < C.log_cap) { C.log[2 * nlog] = stored; C.log[2 * nlog + 1] = need; }
    nlog++;
}

#ifdef ZZ_PROF
#define ZZ_PROF_DECL unsigned long long prof_acc[16] = {0}; unsigned long long prof_last; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_last) :: "memory");
// stamp form of cdna_hip_programming.md section 7: one asm statement, fenced against the scheduler
#define ZZ_T(i) do { unsigned long long _t; __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t) :: "memory"); __builtin_amdgcn_sched_barrier(0); \
    prof_acc[i] += _t - prof_last; prof_last = _t; } while (0)
// diagnostic only: drain outstanding vector-memory operations so that the next stamp prices their latency
#define ZZ_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define ZZ_C(i, v) do { prof_acc[i] += (v); } while (0)
#define ZZ_PROF_FLUSH(P) do { if (threadIdx.x == 0 && (P).prof) for (int _i = 0; _i < 16; ++_i) atomicAdd(&(P).prof[_i], prof_acc[_i]); } while (0)
// one set of counters per wavefront of the workgroup (zz_debug_read_prof_sets)
#define ZZ_PROF_FLUSH_W(P, w) do { if ((threadIdx.x & 63) == 0 && (P).prof) for (int _i = 0; _i < 16; ++_i) atomicAdd(&(P).prof[16 * (w) + _i], prof_acc[_i]); } while (0)
#else
#define ZZ_PROF_DECL
#define ZZ_T(i)
#define ZZ_DRAIN()
#define ZZ_C(i, v)
#define ZZ_PROF_FLUSH(P)
#define ZZ_PROF_FLUSH_W(P, w)
#endif
