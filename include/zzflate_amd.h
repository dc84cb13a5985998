/* zzflate_amd.h -- C ABI of the MI355X-native zzflate encoder path (libzzflate_amd.so).
 *
 * Drop-in boundary for jandevaan/zzflate's encoder entry points (reference zzflate/zzflate.h:8-19):
 *
 *   reference (C++ linkage)                                   this library
 *   ---------------------------------------------------------------------------------------------------
 *   enum Format {Zlib, Gzip, Deflate}          zzflate.h:8     ZZ_ZLIB / ZZ_GZIP / ZZ_DEFLATE (same values)
 *   struct Config {format; level; threaded}    zzflate.h:10-15 zz_config (same 8-byte layout)
 *   ZzFlateEncode(dest,&len,src,n,cfg)         zzflate.h:17    zz_encode()            [+ the C++ symbol itself,
 *   ZzFlateEncodeToCallback(src,n,cfg,fn)      zzflate.h:19    zz_encode_callback()    see include/zzflate.h]
 *   adler32x / combine                         adler.cpp:5-43  zz_adler32 / zz_adler32_combine
 *   crc32                                      crc.h:7         zz_crc32 (+ zz_crc32_combine, new)
 *
 * Plain pointers and sizes only. The *_device entry points take HIP device pointers (what
 * torch.Tensor.data_ptr() returns on ROCm) and a hipStream_t passed as void*.
 *
 * Semantics: `threaded != 0` selects packet mode = the reference's threaded path (zzflate.cpp:97-155) with
 * fixed-size ranges ("packets", default 32 KiB) instead of hardware_concurrency() ranges; every packet is
 * bit-identical to the reference's packet recipe (zzflate.cpp:101-125) wherever that recipe yields a valid
 * DEFLATE encoding, and always valid otherwise. `threaded == 0` asks for the reference's single Encoder over the
 * whole input (zzflate.cpp:84-95): produced on the device too and bit-identical to the reference wherever the
 * reference's stream is a valid encoding of the input (its multi-block level-1 stream is not when a short match crosses a
 * block cut -- defect D12 in DESIGN.md: lengths stop at the block end here), including what
 * depends on where the output goes -- at level 1 the block lengths follow from the room in the caller's buffer
 * (encoder.cpp:331-337; zztest/Test.cpp passes dest = input size) or, through the callback, from the library's
 * 1,000,000-byte chunks (outputbitstream.h:171-201), and the callback receives exactly the reference's chunks. At
 * levels 1..3 that stream is one dependency chain, so it is made by a single wavefront -- a compatibility mode,
 * not a throughput mode. There is no CPU path.
 *
 * Error convention (zzflate.cpp:229-234): *dest_len = ~0 for a bad level or a destination that cannot hold
 * the container header. This library additionally detects a destination that is too small for the stream
 * (the reference silently truncates) and reports it the same way. Functions returning int return 0 on
 * success and a negative ZZ_E_* code otherwise; zz_last_error() gives the message for this thread.
 */
#ifndef ZZFLATE_AMD_H
#define ZZFLATE_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ZZ_ZLIB = 0, ZZ_GZIP = 1, ZZ_DEFLATE = 2 };       /* zzflate.h:8 */
typedef struct { int32_t format; uint8_t level; uint8_t threaded; } zz_config; /* zzflate.h:10-15, sizeof 8 */

enum {
    ZZ_OK = 0,
    ZZ_E_LEVEL = -1,        /* level not in 0..3 (zzflate.cpp:201,230) */
    ZZ_E_NOSPACE = -2,      /* destination too small */
    ZZ_E_HIP = -3,          /* HIP runtime error / no device */
    ZZ_E_ARG = -4,          /* bad argument (packet size, null pointer) */
    ZZ_E_UNSUPPORTED = -5,  /* the device lacks a property the requested mode needs (zz_ctx_set_warm_window, zz_ctx_set_extended_levels);
                               zz_decode_device: a preset dictionary (FDICT) */
    ZZ_E_DATA = -6          /* not a valid stream of the requested format: header, block structure, distance too far back,
                               checksum or ISIZE mismatch, bytes behind the trailer */
};

#define ZZ_DEFAULT_PACKET 32768u
#define ZZ_MAX_PACKET_SIZE 32768u

typedef struct zz_ctx zz_ctx;

/* ---- contexts (device, workspace, timing) ------------------------------------------------------- */
int zz_ctx_create(int device, zz_ctx** out);
void zz_ctx_destroy(zz_ctx* ctx);
/* bytes of device workspace currently held */
uint64_t zz_ctx_workspace_bytes(const zz_ctx* ctx);
/* record HIP events around the encode kernel of each call; read with zz_ctx_last_kernel_ms */
void zz_ctx_enable_timing(zz_ctx* ctx, int on);
/* duration of the last call's dominant (encode) kernel in ms, from HIP events on the launch stream;
 * negative if timing was off */
double zz_ctx_last_kernel_ms(zz_ctx* ctx);

/* Warm window (beyond the reference). The reference's threaded mode gives every range a cold hash
 * table and so loses the matches that would reach back into the previous range; its single Encoder carries the table
 * across blocks (FixHashTable, encoder.cpp:320-327). With a warm window of `bytes` (0..32768) every packet (levels >= 1)
 * starts with the last `bytes` bytes in front of it hashed into its table (every position, per hash the highest), so
 * matches may cross packet boundaries while packets still encode independently. The stream is valid DEFLATE but no
 * longer the reference's threaded stream, hence a separate switch: 0 = off (default). Shards must make the window
 * available as their halo. Env ZZFLATE_WARM_WINDOW sets it for the host entry points. */
int zz_ctx_set_warm_window(zz_ctx* ctx, uint32_t bytes);
/* Levels beyond the reference (BASELINE configs[3] asks for a "level 6 (longer hash chains)" the reference does
 * not have: it rejects every level above 3, zzflate.cpp:201,230-234). Off by default, so that the drop-in keeps that error. When
 * on, levels 4, 5, 6 are accepted by the packet-mode entry points: hash chains of depth 2 / 4 / 8 (four-byte keys) over a window
 * of 8 / 32 / 32 KiB in front of every packet, one-step lazy matching, one dynamic block per packet with code lengths by
 * package-merge. Not comparable with any reference stream; defined by the oracle, checked bit for bit against it,
 * by inflate, and by ratio (mixed corpus: 0.461 at level 3, 0.422 at level 6). Shards must make the window available as their
 * halo. Workspace: 4 bytes per input byte of a call, for at most 1 GiB of input at a time (larger calls go through in batches),
 * and 128 MiB. Env ZZFLATE_EXTENDED_LEVELS=1 switches them on for the host entry points. */
int zz_ctx_set_extended_levels(zz_ctx* ctx, int on);

/* ---- sizes -------------------------------------------------------------------------------------- */
/* worst-case output bytes for n input bytes (container included) */
uint64_t zz_bound(uint64_t n, int format, int level, uint32_t packet_size);

/* ---- host-buffer entry points (drop-in for zzflate.h:17,19) -------------------------------------- */
/* dest_len: in = capacity, out = bytes written or ~0. Packet mode (threaded != 0) fans the input out over every
 * visible GPU (env ZZFLATE_DEVICES = "0,1,..." or "all"; env ZZFLATE_DEVICE = one index), the device analogue of the
 * reference's std::async fan-out over all cores (zzflate.cpp:97-155): buffers longer than one slab (64 MiB, env
 * ZZFLATE_SLAB_MIB) are cut into slabs of whole packets, slab i goes to device i mod D, and on every device H2D,
 * encode and D2H of different slabs overlap. Only two slabs of input and output are resident per device, so the input
 * may be larger than HBM. Re-entrant: concurrent calls (and calls from inside a callback) borrow separate contexts. */
int zz_encode(uint8_t* dest, uint64_t* dest_len, const uint8_t* src, uint64_t n, const zz_config* cfg);
/* callback(user, chunk, bytes) is invoked in order: header, stream chunks of <= 1,000,000 bytes
 * (outputbitstream.h:183), trailer. With threaded == 0 the chunks are the reference's own (see
 * zz_encode_stream_chunks_device). The callback's return value is ignored, as in the reference. Nothing is delivered
 * before the first part of the stream has encoded successfully. */
typedef int (*zz_callback)(void* user, const uint8_t* chunk, uint64_t bytes);
int zz_encode_callback(const uint8_t* src, uint64_t n, const zz_config* cfg, zz_callback cb, void* user);
/* packet size used by the host entry points (env ZZFLATE_PACKET_SIZE overrides the default) */
int zz_set_packet_size(uint32_t packet_size);
uint32_t zz_get_packet_size(void);

/* ---- device-resident entry points ---------------------------------------------------------------- */
/* Whole stream: d_src[0,n) -> d_dst (container header, packets, trailer). *out_len = bytes or ~0.
 * Every single-stream encode entry point below (this one, its two halves, the shard calls, zz_encode_multi_device, the
 * sequential stream and its chunked form, zz_encode_ranges_device) and zz_encode: nothing is written outside d_dst[0, cap),
 * whatever the result. A stream of exactly `cap` bytes fits; one byte less gives ZZ_E_NOSPACE, also where only the trailer
 * does not fit. What lies in d_dst[0, cap) after ZZ_E_NOSPACE is unspecified. A call that is refused, for whatever reason, is
 * still the context's last call: zz_verify_last_device, zz_packet_extent_device and zz_packet_index_device answer ZZ_E_ARG
 * after it, they never describe the call in front of it. */
int zz_encode_device(zz_ctx* ctx, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                     int format, int level, uint32_t packet_size, void* hip_stream);

/* Many independent buffers, one call. Item i = d_srcs[i][0, d_ns[i]) becomes its own complete stream (container header,
 * packets, trailer) in d_dsts[i][0, d_caps[i]); d_out_lens[i] = its length, or ~0 when it does not fit (nothing is
 * written past d_caps[i]; the other items are still complete). Every item's bytes are exactly what
 * zz_encode_device(ctx, d_srcs[i], d_ns[i], d_dsts[i], d_caps[i], .., format, level, packet_size, ..) writes for it alone:
 * an empty item gets one empty final block, an item of at most one packet the reference's single-encoder stream, and no
 * match reaches in front of an item. All five arrays live in device memory. Returns ZZ_OK, ZZ_E_NOSPACE if at least one
 * item did not fit, or the usual errors; nitems == 0 returns ZZ_OK at once, null arrays give ZZ_E_ARG. Levels 0..3, cold
 * packets: ZZ_E_UNSUPPORTED when the context has a warm window or the extended levels switched on (levels 4..6 come through
 * zz_encode_batch_flags_device's own switch, below). At most 2^31 - 1
 * items and 2^31 - 1 packets in all. Synchronous; the host reads back two totals of the plan, whatever nitems is.
 * zz_ctx_last_kernel_ms reports the batch's encode kernels. A batch is not a "last call" for zz_verify_last_device,
 * zz_packet_extent_device and zz_packet_index_device: they return ZZ_E_ARG after it. Workspace: about what a single call
 * over the batch's bytes takes, plus 140 bytes per item and 16 bytes per packet. */
int zz_encode_batch_device(zz_ctx* ctx, uint64_t nitems, const void* const* d_srcs, const uint64_t* d_ns,
                           void* const* d_dsts, const uint64_t* d_caps, uint64_t* d_out_lens,
                           int format, int level, uint32_t packet_size, void* hip_stream);
/* The same call with flags; zz_encode_batch_device is this call with flags = 0. Unknown bits give ZZ_E_ARG.
 * ZZ_BATCH_EXTENDED is the call's own switch for the extended levels 4, 5, 6 (hash chains of depth 2 / 4 / 8, lazy matching,
 * package-merge code lengths): item i becomes exactly the stream zz_encode_device writes for it alone on a context with
 * zz_ctx_set_extended_levels on, at the same format, level and packet size; an empty item gets the empty final block of
 * level 2. The window rule: packet k of an item sees the min(k * packet_size, 8192) bytes in front of it at level 4, and
 * min(k * packet_size, 32768) bytes at levels 5 and 6, all of its own item -- no position in front of an item belongs to
 * its window, whatever lies there in memory. With the switch set, in this order: a warm window on the context gives
 * ZZ_E_UNSUPPORTED; the context's extended switch does not matter (it stays the switch of the single-stream calls); a level
 * outside 0..6 gives ZZ_E_LEVEL; levels 4..6 on a device whose LDS does not serve equal addresses in lane order give
 * ZZ_E_UNSUPPORTED (as zz_ctx_set_extended_levels does); levels 0..3 are the calls as they are without the switch.
 * zz_ctx_last_kernel_ms covers both kernels of the extended levels. Workspace at levels 4..6: a single extended call's over
 * the batch's packets, which counts 4 * packet_size bytes of match words for every packet of a round, however short the
 * packet is, and one CU-owning workgroup per packet -- a batch of very small items pays for full packets. */
enum { ZZ_BATCH_EXTENDED = 1 };
int zz_encode_batch_flags_device(zz_ctx* ctx, uint64_t nitems, const void* const* d_srcs, const uint64_t* d_ns,
                                 void* const* d_dsts, const uint64_t* d_caps, uint64_t* d_out_lens,
                                 int format, int level, uint32_t packet_size, int flags, void* hip_stream);

/* One buffer to one blocked gzip (BGZF) file: what bgzip -d, samtools, tabix, gzip(1) and zz_decode_members_device (its
 * parallel path, no index needed) read, a random-access format (member offset + offset inside the member), and one that
 * concatenates: pieces written with ZZ_MEMBERS_NO_EOF and joined with `cat` are a file.
 * The format rule: d_src[0, n) is cut into blocks of block_size bytes (0 = ZZ_MEMBERS_BLOCK, bgzip's; the last block is
 * shorter; n == 0 gives no blocks). Member i is, in order,
 *   the 18-byte header 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 <BSIZE lo> <BSIZE hi>, BSIZE = the member's bytes - 1;
 *   the body: exactly the raw-deflate stream zz_encode_batch_device(ZZ_DEFLATE, level, packet_size) writes for block i alone
 *     (cold packets, the last one final, no match reaching in front of the block), D bytes -- or, when D > S, the level-0
 *     stream of the same block at the same packet size, S bytes (the stored fallback), so that a file is never longer than
 *     its stored form and no member passes 65,536 bytes;
 *   CRC-32 of the block, then ISIZE, little-endian.
 * Behind the last member comes bgzip's empty member of 28 bytes, unless ZZ_MEMBERS_NO_EOF is set (n == 0 writes that member
 * alone, or nothing). *out_len = the file's bytes.
 * d_member_offsets (optional, device memory, max_offsets entries) receives members + 1 file offsets: each member's first byte,
 * then the offset where the empty last member starts (= the file's length under ZZ_MEMBERS_NO_EOF); they are written
 * whenever the call gets as far as its encode, also when the file then does not fit.
 *   ZZ_E_ARG, before anything is launched: a null context (*out_len = ~0 where there is one), a null d_src with n > 0, a null
 *     d_dst with cap > 0, a null out_len, an unfinished zz_encode_device_async on the context; block_size above 65,536,
 *     packet_size above 32,768, or a pair whose full stored member, 18 + S(block_size, packet_size) + 8, passes 65,536 bytes
 *     (65,280 with packets of 32,768 or 4,096 is accepted, with packets of 1,000 it is not); max_offsets < members + 1; more
 *     than 2^31 - 1 members or packets.
 *   ZZ_E_LEVEL: level outside 0..3.   ZZ_E_UNSUPPORTED: the context has a warm window or the extended levels switched on.
 *   With ZZ_MEMBERS_EXTENDED in flags (the call's own switch, as ZZ_BATCH_EXTENDED of zz_encode_batch_flags_device): levels 0..6.
 *     A member's body at level 4, 5 or 6 is the raw-deflate stream of its block alone at that extended level -- packet k sees
 *     the min(k * packet_size, 8192) bytes (level 4) or min(k * packet_size, 32768) bytes (levels 5, 6) of its own block in
 *     front of it and nothing in front of the block -- or the block's level-0 stream where that is shorter: the rule above
 *     with "levels 0..3" widened. In this order: a warm window on the context gives ZZ_E_UNSUPPORTED; the context's extended
 *     switch does not matter; a level outside 0..6 gives ZZ_E_LEVEL; levels 4..6 on a device with a negative LDS-order verdict
 *     give ZZ_E_UNSUPPORTED. zz_encode_members_bound does not depend on the level or on this bit.
 *   ZZ_E_NOSPACE: the file does not fit cap; *out_len = ~0 and no byte of d_dst is written (decided on the device from the
 *     scanned sizes before any pass stores).
 * Synchronous: the host reads one small record, whatever the member count, and device-side consumers of d_dst wait for the
 * call. Like a batch it is not a "last call" for zz_verify_last_device, zz_packet_extent_device and zz_packet_index_device,
 * and it leaves the decode state alone. Workspace: a batch's over the same blocks, plus 25 bytes per member (levels 4..6:
 * an extended batch's, 4 * packet_size bytes of match words per packet of a round included). */
enum { ZZ_MEMBERS_NO_EOF = 1 };
enum { ZZ_MEMBERS_EXTENDED = 2 };
#define ZZ_MEMBERS_BLOCK 65280u
int zz_encode_members_device(zz_ctx* ctx, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                             int level, uint32_t block_size, uint32_t packet_size, int flags,
                             uint64_t* d_member_offsets, uint64_t max_offsets, void* hip_stream);
/* (host, no device) the largest file zz_encode_members_device can write for these arguments -- every member stored; ~0 for
 * sizes the call refuses */
uint64_t zz_encode_members_bound(uint64_t n, uint32_t block_size, uint32_t packet_size, int flags);
/* (host, no device) the header of a member of member_bytes bytes (1..65536) in all; returns 18 */
int zz_members_header(uint32_t member_bytes, uint8_t out[18]);
/* what the last zz_encode_members_device wrote: its members (the blocks, without the empty last member) and how many of them
 * took the stored fallback (level 0: none -- every member is its level-0 stream). Both are 0 after a refused call and when
 * there has been no call. */
int zz_ctx_last_encode_members_stats(const zz_ctx* ctx, uint64_t* members, uint64_t* stored_members);

/* The same call in two halves: zz_encode_device_async enqueues the whole pipeline on `hip_stream` and returns without
 * waiting; zz_encode_finish waits for it and returns the length (or the error, as zz_encode_device). With two contexts
 * on two streams, call i+1 can be enqueued before call i is finished: its encode kernel fills the CUs call i's last
 * packets leave idle and runs under call i's compaction and result copy. One enqueued call per context at a time. */
int zz_encode_device_async(zz_ctx* ctx, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, int format, int level,
                           uint32_t packet_size, void* hip_stream);
int zz_encode_finish(zz_ctx* ctx, uint64_t* out_len);

/* The reference's sequential whole-buffer stream (threaded == 0, zzflate.cpp:84-95) for device-resident data, in
 * the form ZzFlateEncode gives it (caller-owned buffer of `cap` bytes): level 0 (stored blocks of 65535 bytes,
 * parallel), level 1 (fixed-Huffman blocks; ONE for the whole input when (cap - header - 1) * 8 / 9 - 8 >= n, else as
 * many as encoder.cpp:331-337 cuts for that capacity) and levels 2,3 (dynamic blocks cut at 20,000 records / 500,000
 * bytes, hash table carried across blocks), the latter two produced by a single wavefront: bit-identical to the
 * reference, far slower than packet mode. n < 2 GiB (the reference funnels lengths through int). Where the reference
 * would run out of room and silently leave a truncated stream, ZZ_E_NOSPACE is returned. */
int zz_encode_stream_device(zz_ctx* ctx, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                            int format, int level, void* hip_stream);
/* The reference's OWN threaded == true split (zzflate.cpp:67-78 divideInRanges, :97-155 WriteDeflateStream) for device-resident
 * data: `count` ranges of ceil(n / count) bytes -- std::thread::hardware_concurrency() of them in the reference, the caller's
 * number here --, every range a fresh encoder whose non-final output ends with one stored byte, joined in order; n < 100 * count
 * gives the single encoder's stream (:84). Bit-identical to what ZzFlateEncode(threaded = true) writes on a machine with `count`
 * hardware threads at levels 0, 2, 3 (tests/golden/ranges.json holds such streams); level 1 returns ZZ_E_LEVEL: the reference's
 * threaded level-1 stream does not inflate, use packet mode. One wavefront per range: a compatibility
 * mode (packet mode -- zz_encode_device -- is the throughput mode and cuts <= 32 KiB ranges instead).
 * Host entry points take this path when ZZFLATE_RANGES=<count> is set (threaded != 0, levels 0, 2, 3). n < 2 GiB. */
int zz_encode_ranges_device(zz_ctx* ctx, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                            int format, int level, uint32_t count, void* hip_stream);
/* The same stream in the form ZzFlateEncodeToCallback gives it (zzflate.cpp:197-222): the encoder writes into
 * library-owned chunks of 1,000,000 bytes and opens a new one when the current one is not "enough" for the next block
 * (outputbitstream.h:171-201), which at level 1 also decides the block lengths. d_dst receives header + stream +
 * trailer contiguously; chunk_sizes[0..*nchunks) (up to max_chunks are written) are the byte counts of the chunks in
 * order, i.e. the sizes the reference's callback sees between the header call and the trailer call. */
int zz_encode_stream_chunks_device(zz_ctx* ctx, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                                   int format, int level, uint64_t* chunk_sizes, uint32_t max_chunks, uint32_t* nchunks,
                                   void* hip_stream);

/* One shard of a stream (multi-GPU: ranks own contiguous packet ranges). d_src points at the shard's first
 * byte; `halo` bytes in front of it are readable input of the same stream (level >= 2 backward match
 * extension reads up to 258 of them; pass 0 for the first shard). No header/trailer is written; the shard's
 * checksum partial comes back for zz_adler32_combine / zz_crc32_combine:
 *   checksum == ZZ_ZLIB: cks = Adler-32 of the shard with start value 0 ((b<<16)|a)
 *   checksum == ZZ_GZIP: cks = CRC-32 of the shard;   ZZ_DEFLATE: none. */
int zz_encode_shard_device(zz_ctx* ctx, const void* d_src, uint64_t n, uint64_t halo, int is_last_shard,
                           void* d_dst, uint64_t cap, uint64_t* out_len, uint32_t* cks, int checksum,
                           int level, uint32_t packet_size, void* hip_stream);

/* The shard call in two halves (as zz_encode_device_async / zz_encode_finish), for ranks that enqueue the next step's shard
 * before the previous one's size and checksum have been exchanged. */
int zz_encode_shard_device_async(zz_ctx* ctx, const void* d_src, uint64_t n, uint64_t halo, int is_last_shard, void* d_dst,
                                 uint64_t cap, int checksum, int level, uint32_t packet_size, void* hip_stream);
int zz_encode_shard_finish(zz_ctx* ctx, uint64_t* out_len, uint32_t* cks, int checksum);

/* Fan-out and join over several GPUs of ONE process, for data already resident on them -- WriteDeflateStream's
 * std::async fan-out and in-order memmove join (zzflate.cpp:97-155) with devices for threads and xGMI peer copies for
 * memmove; no torch, no RCCL. Shard i = d_src[i][0, n[i]) lives on the device of ctxs[i] (one context per shard; a device
 * may appear more than once); the shards are consecutive ranges of one stream, every one but the last a whole number of
 * packets; halo[i] (halo may be NULL = all 0) = readable bytes of the stream in front of d_src[i] on that device, as
 * zz_encode_shard_device wants them. All shards are encoded concurrently; each is pulled to its final offset in d_dst --
 * on the device of ctxs[0], where shard 0 is encoded in place -- with hipMemcpyPeerAsync as soon as the shards in front of
 * it have finished; checksums are folded on the host; header and trailer are written. *out_len = bytes or ~0. */
int zz_encode_multi_device(zz_ctx* const* ctxs, int nshards, const void* const* d_src, const uint64_t* n, const uint64_t* halo,
                           void* d_dst, uint64_t cap, uint64_t* out_len, int format, int level, uint32_t packet_size);

/* Self-verification: inflates, on the device, every packet of the stream the LAST zz_encode_device /
 * zz_encode_shard_device call on this context produced, and compares with that call's input (both buffers must still
 * be in place). *bad_packets = packets that do not decode to their input, *first_bad_packet = the lowest such packet
 * (~0 if none). A checker for tests, benchmarks and deployments that want an end-to-end guarantee; the reference has
 * no decoder (decoder.h is an empty stub). */
int zz_verify_last_device(zz_ctx* ctx, uint64_t* bad_packets, uint64_t* first_bad_packet, void* hip_stream);

/* Random access: where packet k (input bytes [k*packet_size, (k+1)*packet_size)) of the stream produced by the LAST
 * zz_encode_device / zz_encode_shard_device call on this context lies. *offset counts from the first byte of the
 * DEFLATE stream (behind the container header), *bytes is the packet's length. Packets are byte-aligned runs of complete
 * blocks (zzflate.cpp:101-125) that start with an empty bit buffer and fresh codes. At levels 0 and 1 with cold packets
 * each can be inflated on its own. At levels >= 2 a match may reach in front of the packet's start (the backward
 * extension, encoder.cpp:404; warm windows and levels 4..6 up to 32 KiB back), so a packet needs the bytes in front of
 * it -- zz_decode_device resolves such references across packets. */
int zz_packet_extent_device(zz_ctx* ctx, uint64_t packet, uint64_t* offset, uint64_t* bytes, void* hip_stream);

/* ---- decode (beyond the reference, whose decoder.h is an empty stub) ------------------------------------------------
 * The packet index of the LAST zz_encode_device / zz_encode_shard_device call on this context: entries = npk + 1
 * offsets counted from the first DEFLATE byte, index[npk] = stream bytes (level 0 included; its offsets are arithmetic;
 * an empty input's one empty block counts as a packet). *entries is set even when max_entries is too small
 * (ZZ_E_NOSPACE). Small (8 bytes per packet); callers that store a stream can store it beside it. */
int zz_packet_index_device(zz_ctx* ctx, uint64_t* d_index, uint64_t max_entries, uint64_t* entries, void* hip_stream);

/* d_src[0, src_len) = a zlib / gzip / raw stream -> d_dst; *out_len = decompressed bytes.
 *   packet_size 1..32768 and d_index != NULL : packets at the given offsets, decoded in parallel
 *   packet_size 1..32768 and d_index == NULL : packet starts found on the device (after every 01 00 FE FF), then as above
 *   packet_size 0                            : any single-member RFC 1950/1951/1952 stream, serial
 * Every valid stream decodes to its bytes whatever packet_size and d_index say: they decide speed, not the result (an
 * index or a packet size that does not fit the stream sends the call to the serial path). The trailer (Adler-32, or
 * CRC-32 and ISIZE) is checked on the device; ZZ_E_DATA for an invalid stream, ZZ_E_NOSPACE when the output does not
 * fit `cap` (nothing is written past it), ZZ_E_UNSUPPORTED for a preset dictionary. A shard that is not the first
 * refers to bytes in front of it: ZZ_E_DATA. d_index holds `entries` int64 offsets in device memory.
 * Cost of errors: a packet-mode stream whose packets all decode but whose output exceeds `cap` gives ZZ_E_NOSPACE at
 * the parallel rate. Any other failure of the parallel paths -- a corrupt byte, a truncated stream, bytes behind the
 * trailer, an index that does not describe the stream -- is decided by the serial path, which runs at a few MB/s: a
 * damaged multi-GiB stream takes minutes to be refused.
 * Workspace: at most ~270 MiB (4 bytes per output byte of a 64 MiB batch, 20 bytes per packet of a batch); discovery adds
 * 20 bytes per candidate, at most 4 Mi candidates. Synchronous, like zz_encode_device. */
int zz_decode_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, void* d_dst, uint64_t cap, uint64_t* out_len,
                     int format, uint32_t packet_size, const uint64_t* d_index, uint64_t entries, void* hip_stream);

/* ---- any stream, decoded in parallel from a point index ----------------------------------------------------------------
 * A stream this library did not write (gzip, zlib.compress, pigz, libdeflate, ..) has no packets; without help it takes
 * zz_decode_device's serial path. Its blocks, though, decode independently once their starts are known, and what crosses a
 * block start -- matches up to 32 KiB back -- is what zz_decode_device's rounds already resolve. The POINT INDEX says where:
 * `entries` = segments + 1 rows of two little-endian uint64, (in_bit, out_byte). in_bit counts from the first DEFLATE byte
 * (behind the container header); row 0 is (0, 0); row k is the header bit of a block (its BFINAL bit) and the decoded bytes in
 * front of it; the last row is (the bit behind the final block, the decoded length). in_bit ascends strictly, out_byte ascends
 * (a segment may decode to nothing, it never consumes nothing). 16 bytes per segment and no window copies: about 128 KiB for
 * a GiB at the default spacing.
 *
 * zz_points_index_host builds it: ONE sequential pass over src[0, src_len) in HOST memory, no GPU, no context, the decoded
 * bytes not kept (a 64 KiB ring is the window). A point is recorded at the first block boundary at or behind every multiple
 * of `spacing` decoded bytes (spacing >= 1; spacing 1: every block). The container header and the trailer (Adler-32, or CRC-32
 * and ISIZE) are checked: ZZ_E_DATA for an invalid stream, ZZ_E_UNSUPPORTED for a preset dictionary, as zz_decode_device gives
 * them. *entries and *out_len are set for every valid stream, also when max_entries is too small (ZZ_E_NOSPACE, nothing
 * written to points). ZZ_POINTS_SPACING_DEFAULT gives a GiB two segments per resident wavefront (4,096 of them): derived, not
 * tuned -- measured on 512 MiB streams of host zlib, a spacing of 32768 decodes about twice as fast, because a 64 MiB batch then
 * holds more segments. */
#define ZZ_POINTS_SPACING_DEFAULT 131072ull
int zz_points_index_host(const uint8_t* src, uint64_t src_len, int format, uint64_t spacing, uint64_t* points,
                         uint64_t max_entries, uint64_t* entries, uint64_t* out_len);

/* zz_decode_device for a stream with a point index: d_src and d_dst in device memory, `points` (entries rows) in HOST memory --
 * the builder makes it there, it is small, and the call walks it batch by batch. One wavefront decodes one segment straight
 * into d_dst; bytes that copy from in front of their segment are finished by the rounds; the trailer is checked on the device.
 * The index is never trusted: rows that are not an index of the shape above, a segment that does not begin at a block header,
 * does not end at its row's bit or does not decode to exactly its row's bytes, or a checksum mismatch send the call to the
 * serial path, which decides the result -- every valid stream decodes to its bytes whatever the index says; it decides speed,
 * not the result. That includes a destination smaller than the stream: the index's own claim about the length is not
 * evidence, so ZZ_E_NOSPACE comes from the serial path, at its rate (a few MB/s). Results as zz_decode_device: ZZ_E_DATA,
 * ZZ_E_UNSUPPORTED, ZZ_E_NOSPACE; nothing is written behind `cap`. ZZ_E_ARG before anything is launched: a null context,
 * source, out_len or points, fewer than 2 entries, a format outside 0..2, an unfinished zz_encode_device_async.
 * zz_ctx_last_decode_path gives ZZ_DECODE_POINTS (or ZZ_DECODE_SERIAL), zz_ctx_last_decode_stats the pending bytes and rounds.
 * Workspace: zz_decode_device's batch (4 bytes and one bit per output byte of at most 64 MiB, 8 bytes per 32 KiB tile) plus
 * 32 bytes per segment of a batch. Synchronous; the host waits once or twice per batch. */
int zz_decode_points_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, void* d_dst, uint64_t cap, uint64_t* out_len,
                            int format, const uint64_t* points, uint64_t entries, void* hip_stream);

/* The point index built ON THE DEVICE, for a stream met for the first time: block starts are found in the compressed bytes in
 * parallel instead of being reached one after the other. D = the bytes behind the container header; it is cut into chunks of
 * chunk_bytes. In every chunk but the first, a kernel looks for the lowest bit at which a NON-FINAL DYNAMIC block header stands
 * that passes every check the decoder makes on one (the candidates; chunk 0's is bit 0). The stretch from every candidate to the
 * next is then measured in one launch -- decoded and counted, no byte written -- and the stretches are chained from bit 0: only
 * candidates reached over block boundaries from bit 0 become rows; a candidate the chain does not meet is dropped and the gap it
 * leaves is measured in a further round. So the rows are: (0, 0); (p, decoded bytes in front of p) for every candidate p on the
 * stream's true chain of blocks; (the bit behind the final block, the decoded length) -- thinned by zz_points_index_host's rule
 * when spacing > 1 (an inner row is kept only if it is the first at or behind a multiple of `spacing` decoded bytes). The result
 * depends on the stream, chunk_bytes and spacing only. Stored, fixed and final blocks are not searched for: a stream made of those
 * gets few rows or none between the first and the last, and decodes as slowly as with any sparse index.
 *
 * `points` is HOST memory, exactly what zz_decode_points_device takes; zz_points_index_bound(src_len, chunk_bytes) rows always
 * suffice (chunks + 1; 0 for chunk_bytes < 16). *entries and *out_len are set also when max_entries is too small (ZZ_E_NOSPACE,
 * nothing written to points), as zz_points_index_host has it.
 *
 * What is checked: the container header as zz_decode_device reads it (ZZ_E_UNSUPPORTED for a preset dictionary); the block
 * structure along the true chain; that exactly the trailer's length lies behind the final block; for gzip, ISIZE against the
 * decoded length: ZZ_E_DATA. What is NOT checked: the checksum and the match distances -- no byte is produced. ZZ_OK here is NOT
 * a verdict on the stream: zz_decode_points_device gives that, and refuses a stream that this call indexed although its checksum
 * is wrong or a distance reaches too far back.
 *
 * ZZ_E_ARG before anything is launched: a null context, source, entries or out_len; chunk_bytes < 16 or spacing < 1; a format
 * outside 0..2; an unfinished zz_encode_device_async. Workspace: 32 bytes per chunk and nothing per output byte. The context's
 * "last decode" state is not touched. Synchronous; the host reads the chunks' records once and each round's records once. */
#define ZZ_POINTS_CHUNK_DEFAULT 16384ull   /* compressed bytes per searched chunk; derived (32 KiB of decoded text at ratio ~0.4, the spacing DESIGN.md 17 measured best), not tuned */
uint64_t zz_points_index_bound(uint64_t src_len, uint64_t chunk_bytes);
int zz_points_index_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format, uint64_t chunk_bytes, uint64_t spacing,
                           uint64_t* points, uint64_t max_entries, uint64_t* entries, uint64_t* out_len, void* hip_stream);
/* what the last zz_points_index_device did: the candidates (bit 0 included), those of them that were dropped, and the rounds
 * (launches of the measuring kernel; a stream whose candidates all lie on its chain needs one) */
int zz_ctx_last_points_index_stats(const zz_ctx* ctx, uint64_t* candidates, uint64_t* dropped, uint32_t* rounds);

/* Many independent streams back to their bytes, one call: the mirror image of zz_encode_batch_device. Item i =
 * d_srcs[i][0, d_src_lens[i]) -- one complete zlib / gzip / raw stream: any single-member RFC 1950 / 1951 / 1952 stream,
 * packet-mode or not, any level, written by this library or another -- is decoded into d_dsts[i][0, d_caps[i]);
 * d_out_lens[i] = its decoded bytes, or ~0; d_status[i] (d_status may be NULL) = ZZ_OK, ZZ_E_DATA (header, block structure,
 * distance, truncated, bytes behind the trailer, checksum or ISIZE mismatch), ZZ_E_NOSPACE (the output does not fit
 * d_caps[i]) or ZZ_E_UNSUPPORTED (preset dictionary). Nothing is read outside an item's source or written outside its
 * destination, and an item that fails leaves the others complete. All six arrays live in device memory. Returns ZZ_OK
 * when every item decoded; otherwise ZZ_E_DATA if any item's status is ZZ_E_DATA or ZZ_E_UNSUPPORTED, else ZZ_E_NOSPACE.
 * nitems == 0 returns ZZ_OK at once; a null context, null arrays, a format outside 0..2, more than 2^31 - 1 items or an
 * unfinished zz_encode_device_async on the context give ZZ_E_ARG before anything is launched. Synchronous; the host reads
 * back two failure counters, whatever nitems is. Workspace: a few counters.
 * One item is decoded by ONE wavefront (container, blocks, trailer and checksum), the wavefronts dealing themselves the items
 * from a counter: an item decodes at a few MB/s, and the call is fast when the batch holds at least as many items as the GPU
 * holds wavefronts (about 4,096); a stream of hundreds of MiB belongs to zz_decode_device. The call leaves the context's
 * "last call" and "last decode" state alone: zz_ctx_last_decode_*, zz_verify_last_device and zz_packet_index_device answer
 * after it as they did before it. */
int zz_decode_batch_device(zz_ctx* ctx, uint64_t nitems, const void* const* d_srcs, const uint64_t* d_src_lens,
                           void* const* d_dsts, const uint64_t* d_caps, uint64_t* d_out_lens, int32_t* d_status,
                           int format, void* hip_stream);

/* Random access into a stored stream: decoded bytes [first, first + nbytes) of a packet-mode stream, from the stream and its
 * packet index alone. d_src[0, src_len) is the WHOLE zlib / gzip / raw stream, d_index its `entries` = packets + 1 offsets as
 * zz_packet_index_device or zz_ctx_last_decode_index_device return them (the index is required: finding packet starts needs the
 * whole stream and stays with zz_decode_device), packet_size 1..32768 the one it was written with. With L the stream's decoded
 * length, d_dst[0, m) receives bytes [first, first + m), m = min(nbytes, L - first) -- the range is clipped at the stream's end,
 * m = 0 for L <= first < packets * packet_size -- and *out_len = m. Nothing is written outside d_dst[0, min(m, cap)).
 *   ZZ_E_ARG, before anything is launched: a null context, source, index or out_len (or a null d_dst with cap > 0); packet_size
 *     outside 1..32768; a format outside 0..2; entries < 2; first >= (entries - 1) * packet_size; first + nbytes overflows; an
 *     unfinished zz_encode_device_async on the context. nbytes == 0 with arguments that pass returns ZZ_OK and *out_len = 0 at once.
 *   ZZ_E_NOSPACE: m > cap; *out_len = ~0, bytes past cap are untouched.   ZZ_E_UNSUPPORTED: a preset dictionary (FDICT).
 *   ZZ_E_DATA: a bad container header; index[0] != 0 or index[last] not the stream's DEFLATE length; a decoded packet that is
 *     not what the index says (exactly packet_size bytes, ending at the next start, BFINAL on the last packet only) or that
 *     refers to bytes in front of the stream.
 * What is decoded: the packets the range touches and a look-back in front of them, for bytes whose match source lies in an
 * earlier packet; when a byte of the range still points in front of the decoded packets, the call repeats with four times the
 * look-back. The cost is bounded by the packets touched -- there is no serial path, so a damaged packet is
 * refused at the parallel rate -- and a call never takes less than one wavefront needs for one packet.
 * NOT CHECKED: the trailer's checksum (Adler-32, CRC-32, ISIZE). It covers bytes this call never decodes, so a corrupt byte
 * that leaves a packet's structure intact (a changed literal, a changed stored byte) comes back as a wrong byte; packets
 * outside the decoded ones are not looked at at all. zz_decode_device checks the whole stream; zz_decode_range_checked_device
 * checks every packet this read returns bytes from, against a sidecar that it first holds to the trailer.
 * Workspace: as zz_decode_device's batch plus one byte per output byte of a batch (64 MiB). Synchronous. Leaves the
 * context's "last call" and "last decode" state alone, as zz_decode_batch_device does. */
int zz_decode_range_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format, uint32_t packet_size,
                           const uint64_t* d_index, uint64_t entries, uint64_t first, uint64_t nbytes,
                           void* d_dst, uint64_t cap, uint64_t* out_len, void* hip_stream);
/* what the last successful zz_decode_range_device did: the first packet it decoded (the range's first packet minus the final
 * look-back), the packets decoded in the final attempt, the attempts, and the bytes phase 1 left pending in the final attempt */
int zz_ctx_last_decode_range_stats(const zz_ctx* ctx, uint64_t* first_packet, uint64_t* packets,
                                   uint32_t* attempts, uint64_t* pending_bytes);

/* Many reads of one stored stream in one call: read r = decoded bytes [d_firsts[r], d_firsts[r] + d_nbytes[r]) into
 * d_dsts[r][0, d_caps[r]), exactly what zz_decode_range_device gives that read alone, but the nranges reads share one set of
 * launches. The stream, its index, format and packet_size are as zz_decode_range_device takes them; the six arrays of nranges
 * entries live in DEVICE memory (d_status may be NULL). With L the stream's decoded length, d_out_lens[r] = m = min(nbytes,
 * L - first) (0 for a start behind the end inside the last packet's span, 0 with ZZ_OK for nbytes == 0); nothing is written
 * outside d_dsts[r][0, min(m, cap)). A read whose status is not ZZ_OK has d_out_lens[r] = ~0 and the first cap bytes of its
 * destination are unspecified; it leaves every other read complete.
 *   d_status[r]: ZZ_OK; ZZ_E_ARG: first >= (entries - 1) * packet_size, or first + nbytes overflows (the arrays live on the
 *     device, so these are refused there); ZZ_E_NOSPACE: m > cap; ZZ_E_DATA: a packet this read decodes is not what the index
 *     says or refers to bytes in front of the stream; ZZ_E_UNSUPPORTED: the read's packets plus look-back exceed one batch (64 MiB
 *     of output, 2^18 packets), at first or after the look-back has grown -- such a read belongs to zz_decode_range_device,
 *     which carries bytes from batch to batch; this call does not.
 *   Returns ZZ_OK when every read is ZZ_OK; otherwise ZZ_E_DATA if any read is, else ZZ_E_UNSUPPORTED, else ZZ_E_ARG, else
 *     ZZ_E_NOSPACE.
 *   ZZ_E_ARG, before anything is launched: a null context, source, index, d_firsts, d_nbytes, d_dsts, d_caps or d_out_lens;
 *     packet_size outside 1..32768; a format outside 0..2; entries < 2; nranges > 2^31 - 1; an unfinished zz_encode_device_async
 *     on the context. nranges == 0 with arguments that pass returns ZZ_OK at once.
 *   Failures of the call itself, after the host reads zz_decode_range_device makes: a bad container header (ZZ_E_DATA), a preset
 *     dictionary (ZZ_E_UNSUPPORTED), index[0] != 0 or index[last] not the stream's DEFLATE length (ZZ_E_DATA); every d_status[r]
 *     is then that code and every d_out_lens[r] = ~0.
 * Reads may overlap each other (each decodes its own copy of the packets); destinations that overlap are the caller's error.
 * NOT CHECKED: the trailer's checksum (Adler-32, CRC-32, ISIZE), for zz_decode_range_device's reason: it covers bytes this call
 * never decodes. zz_decode_ranges_checked_device is the same call with every returned packet checked against a sidecar.
 * How: every read's packets and look-back form a segment on a stage; the segments of many reads go through phase 1 and the
 * rounds together, a wave of at most two batches of packets at a time; a read that still points in front of its segment comes
 * back in the next attempt with four times the look-back, the others are finished. Per attempt the host
 * reads a fixed number of words, whatever nranges is.
 * Workspace: at most twice zz_decode_range_device's (a wave holds fewer than two batches of packets: per packet its bytes, four
 * bytes of pointer per byte, the bitmap, 44 bytes) plus 48 bytes per read; sized by the call's largest wave. Synchronous.
 * Leaves the context's "last call", "last decode" and zz_ctx_last_decode_range_stats state alone. */
int zz_decode_ranges_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format, uint32_t packet_size,
                            const uint64_t* d_index, uint64_t entries,
                            uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                            void* const* d_dsts, const uint64_t* d_caps,
                            uint64_t* d_out_lens, int32_t* d_status, void* hip_stream);
/* what the last zz_decode_ranges_device did: stage packets decoded, summed over its attempts; the attempts; the reads that
 * needed more than one attempt; the waves, summed over its attempts */
int zz_ctx_last_decode_ranges_stats(const zz_ctx* ctx, uint64_t* packets, uint32_t* attempts,
                                    uint64_t* retried_ranges, uint32_t* waves);

/* ---- checked range reads: a per-packet checksum sidecar ---------------------------------------------------------------
 * The SIDECAR of a stream written with packet size P from L decoded bytes: max(1, ceil(L / P)) little-endian uint32 values in
 * device memory, entry k = the checksum of decoded bytes [k * P, min((k + 1) * P, L)) as zlib computes it -- adler32 (start
 * value 1) for ZZ_ZLIB, crc32 for ZZ_GZIP and ZZ_DEFLATE; an empty stream has one entry, 1 or 0. Stored beside the stream and
 * its index (12 bytes per packet together) it lets a range read verify what it returns.
 *
 * zz_packet_checksums_device computes the sidecar of ANY device buffer d_data[0, n): the input before it is encoded, or a
 * decoded copy. *entries is set even when max_entries is too small (ZZ_E_NOSPACE, nothing written: zz_packet_index_device's
 * convention). ZZ_E_ARG: a null context, entries or d_cks (or null d_data with n > 0), packet_size outside 1..32768, a format
 * outside 0..2, more than 2^31 - 1 packets. Stateless: it does not depend on the context's last call and leaves the "last call",
 * "last decode" and range-stats state alone. Synchronous. Workspace: 8 bytes per packet. */
int zz_packet_checksums_device(zz_ctx* ctx, const void* d_data, uint64_t n, uint32_t packet_size, int format,
                               uint32_t* d_cks, uint64_t max_entries, uint64_t* entries, void* hip_stream);

/* zz_decode_range_device with every packet it returns bytes from verified. d_cks is the stream's sidecar (entries - 1 values),
 * total_len its decoded length L (the caller knows it; gzip also stores it). Arguments, clipping, m, cap, look-back growth,
 * batches, zz_ctx_last_decode_range_stats and "nothing written outside d_dst[0, min(m, cap))" are zz_decode_range_device's.
 *   ZZ_E_ARG on top, before anything is launched: d_cks null; entries - 1 != max(1, ceil(total_len / packet_size)); more than
 *     2^31 - 1 packets.
 *   The sidecar is never trusted. In every call its entries are folded in packet order on the device (the last packet's length
 *     from total_len) and the fold is held to the stream's own trailer: Adler-32 for zlib; CRC-32 and ISIZE (against total_len mod
 *     2^32) for gzip. A mismatch, or an entry no packet can have: ZZ_E_DATA, *out_len = ~0, no destination byte written.
 *     ZZ_DEFLATE HAS NO TRAILER: there nothing vouches for the sidecar but the caller who stored it -- the call then proves that
 *     the bytes match the caller's sidecar, not that the sidecar matches what was once encoded.
 *   Every packet [first / P, ...) the range touches is summed whole on the device after it is decoded -- its length is what the
 *     decoder produced, not what the host expects -- and compared with its entry; the stream's last packet must also hold
 *     exactly total_len - (packets - 1) * P bytes. Look-back packets are not summed: none of their bytes is returned. Any
 *     mismatch: ZZ_E_DATA, *out_len = ~0; earlier batches of a long range may already have been copied, so d_dst[0, min(m, cap))
 *     is unspecified, as after any failed read.
 *   A packet with an unresolved byte cannot be summed, so a byte that points in front of the decoded packets sends the call
 *     back for a longer look-back when it lies anywhere in a touched packet, not only inside [first, first + m): the returned
 *     bytes are the same, the look-back may grow one step earlier than the unchecked call's.
 * Cost on top of the unchecked call: one pass over the touched packets on the stage and an O(packets) fold of the sidecar; the
 * host reads one more word per call. Workspace on top: 8 bytes per packet of the stream and 8 per packet of a batch. */
int zz_decode_range_checked_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format, uint32_t packet_size,
                                   const uint64_t* d_index, uint64_t entries,
                                   const uint32_t* d_cks, uint64_t total_len,
                                   uint64_t first, uint64_t nbytes,
                                   void* d_dst, uint64_t cap, uint64_t* out_len, void* hip_stream);

/* zz_decode_ranges_device with every returned packet verified; d_cks and total_len as zz_decode_range_checked_device takes them,
 * and its ZZ_E_ARG cases on top of zz_decode_ranges_device's. The sidecar is held to the trailer once per call: on failure
 * every d_status[r] = ZZ_E_DATA, every d_out_lens[r] = ~0, nothing is written and the call returns ZZ_E_DATA. Per read: the
 * widened window, and its touched packets summed after the rounds of its wave; a mismatch is charged to that read alone
 * (ZZ_E_DATA, ~0, its destination not copied) and leaves the others complete. Status precedence, waves, attempts, stats and the
 * fixed number of words the host reads per attempt are zz_decode_ranges_device's. For ZZ_DEFLATE see above. */
int zz_decode_ranges_checked_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format, uint32_t packet_size,
                                    const uint64_t* d_index, uint64_t entries,
                                    const uint32_t* d_cks, uint64_t total_len,
                                    uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                    void* const* d_dsts, const uint64_t* d_caps,
                                    uint64_t* d_out_lens, int32_t* d_status, void* hip_stream);

/* A file of gzip members back to back (RFC 1952 2.2): what `cat a.gz b.gz`, an append-mode gzip writer and bgzip / BAM / tabix
 * (BGZF) write, and what gzip(1), zlib's gzread and Python's gzip.decompress read. d_src[0, src_len) holds one or more members;
 * each is judged exactly as zz_decode_batch_device judges a single gzip item, the first byte behind a member's trailer is the
 * next member's 1f or the end of the file, and d_dst[0, *out_len) receives the members' bytes one after the other. Zero
 * padding between or behind members is NOT accepted (zlib's verdict, not gzip(1)'s leniency), nor is an empty file.
 * Paths (zz_ctx_last_decode_members_stats):
 *   1  blocked: every member announces its length in a `BC` extra subfield (anywhere among its subfields), the headers found
 *      by a pass over the source form one chain from offset 0 to src_len, checked in parallel; the members are then decoded as a
 *      batch, one wavefront each, at zz_decode_batch_device's rate -- fast from a few thousand members on
 *   2  blocked, but a member holds bytes that look like such a header (a blocked file stored inside a blocked file): the chain
 *      is walked from offset 0 by one lane, one dependent load per member, then decoded as in path 1
 *   3  serial: members without `BC`, a chain that cannot be walked, and every file in which a member fails: ONE wavefront
 *      decodes member after member at a few MB/s, like packet_size 0 of zz_decode_device
 * The paths decide speed, never the result: the serial path is the definition, and the blocked paths answer only what it
 * would. Verdict: members are judged in file order and the first one that fails decides -- ZZ_E_DATA if it is invalid (header,
 * blocks, truncation, CRC-32, ISIZE, a byte that is not a header behind a trailer, src_len == 0), ZZ_E_NOSPACE if its bytes
 * pass `cap` before it is found invalid; nothing is written outside d_dst[0, cap). *out_len = ~0 on failure.
 * Cost of errors: a blocked file that is merely too large for `cap` is refused at the parallel rate plus ONE member at the
 * serial rate (the member that ran out of room is judged again as the serial path reads it); any other failure is
 * decided by the serial path, so a damaged multi-GiB file takes minutes to be refused.
 * ZZ_E_ARG, before anything is launched: a null context, a null d_src with src_len > 0, a null d_dst with cap > 0, a null
 * out_len, an unfinished zz_encode_device_async on the context.
 * Workspace: 12 bytes per 4 KiB of source and 52 bytes per header-like offset found (members or not). Limits: the blocked paths
 * take at most 2^31 - 1 members (a file with more header-like offsets goes to the serial path). Synchronous; the host reads
 * a fixed handful of numbers, whatever the member count. Leaves the context's "last call" and "last decode" state alone, as
 * zz_decode_batch_device does. */
int zz_decode_members_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, void* d_dst, uint64_t cap,
                             uint64_t* out_len, void* hip_stream);
/* what the last zz_decode_members_device did: the members it decoded (on failure: those in front of the deciding one when the
 * serial path decided, else those dealt), the header-like offsets the blocked path found (candidates), and the path:
 * 1 blocked, chain verified in parallel; 2 blocked, chain walked; 3 serial (0: no call yet, or refused before a path was taken) */
int zz_ctx_last_decode_members_stats(const zz_ctx* ctx, uint64_t* members, uint64_t* candidates, int* path);

/* The index of a blocked gzip (BGZF) file, made on the device from the file alone. An index is `entries` = members + 1 pairs of
 * uint64 in DEVICE memory, one array of 2 * entries words: d_index[2j] is the file offset of member j's first byte,
 * d_index[2j + 1] the decoded offset of its first byte; the last pair is (the offset behind the last member, the decoded length
 * L). This is bgzip's .gzi content with its omitted first and last pairs put back; an empty member (bgzip's 28-byte last one,
 * or one in the middle of a file) is a member like any other, with two equal decoded offsets.
 * How: mark, scan, fill, check and hop exactly as zz_decode_members_device makes them (its paths 1 and 2), then a scan of the
 * members' ISIZE. NOTHING IS DECODED: the decoded offsets are the members' own claims, and a read through the index
 * (zz_decode_members_ranges_device) is what checks them.
 *   *entries = members + 1 is set even when max_entries is too small; the call then returns ZZ_E_NOSPACE and writes nothing
 *     (as zz_packet_index_device: call with max_entries 0 for the size).
 *   ZZ_E_UNSUPPORTED: the file is not blocked -- no member announces its length, or the chain from offset 0 cannot be walked
 *     (members without `BC`, `cat a.gz b.gz`). Indexing such a file means decoding it, which zz_decode_members_device does.
 *     zz_members_find_device below makes the same index for such a file by measuring its members in parallel.
 *   ZZ_E_DATA: src_len == 0.
 *   ZZ_E_ARG, before anything is launched: a null context, a null d_src with src_len > 0, a null d_index with max_entries > 0,
 *     null entries, an unfinished zz_encode_device_async on the context.
 * Workspace: zz_decode_members_device's mark pass, 12 bytes per 4 KiB of source and 12 bytes per header-like offset. Synchronous.
 * Leaves the context's "last call", "last decode" and zz_ctx_last_decode_members_stats state alone. */
int zz_members_index_device(zz_ctx* ctx, const void* d_src, uint64_t src_len,
                            uint64_t* d_index, uint64_t max_entries,
                            uint64_t* entries, void* hip_stream);

/* The same index for ANY file of gzip members -- `cat a.gz b.gz`, append-mode logs, WARC files, whatever gzip.open(.., "ab")
 * wrote: members that announce no length, so their ends are found by measuring. The result is defined by the file alone
 * (DESIGN.md 22):
 *   candidates  offset 0, and every offset i >= 20 where a gzip header stands that zz_decode_members_device would accept there
 *               and that leaves ten bytes behind it; the first byte of every member of a valid file is one
 *   measure     a candidate is decoded as a member WITHOUT WRITING A BYTE: header, blocks through the final one, eight bytes of
 *               trailer whose ISIZE equals the low 32 bits of the byte count. That gives its length in the file and, exactly,
 *               its decoded length. CRC-32 and match distances are not judged: there are no bytes yet.
 *   walk        from offset 0 over the measured lengths. It must reach src_len exactly, over candidates whose measures
 *               succeeded; candidates it steps over (headers stored inside a member) are dropped.
 * The index has zz_members_index_device's format and size protocol: members + 1 pairs (file offset, decoded offset), the last
 * (src_len, L); *entries is set even when max_entries is too small, and the call then returns ZZ_E_NOSPACE and writes nothing.
 * Unlike that index its decoded offsets are measured, not claimed.
 *   limit_bytes  a measure that does not start at offset 0 may start anywhere, so it gives up once it has consumed limit_bytes of
 *     the file; the walk then runs the measures it needs again without a limit (two rounds at most). The result does not depend
 *     on limit_bytes; only the time does. 0 means ZZ_MEMBERS_FIND_LIMIT_DEFAULT.
 *   ZZ_OK is not a verdict on checksums: a read through the index (zz_decode_members_ranges_device) or a decode
 *     (zz_decode_members_found_device) gives that.
 *   ZZ_E_DATA: the walk breaks -- src_len == 0, a member that cannot be measured (header, blocks, truncation, ISIZE), or a byte
 *     that is no header behind a trailer.
 *   ZZ_E_UNSUPPORTED: more than 2^31 - 1 candidates (zz_decode_members_device still decodes such a file).
 *   ZZ_E_ARG, before anything is launched: a null context, a null d_src with src_len > 0, a null d_index with max_entries > 0,
 *     null entries, an unfinished zz_encode_device_async on the context.
 * Cost: one pass over the file at memory bandwidth, then every candidate's blocks decoded once by one wavefront (a member is the
 * unit: a file of two huge members gains a factor of two and no more). A header field that runs to the next zero byte (FNAME,
 * FCOMMENT) is followed from every candidate that has one.
 * Workspace: 12 bytes per 4 KiB of source and 45 bytes per candidate, sized from the count the device reports. Synchronous; the
 * host reads 32 bytes per candidate and round. Leaves the context's "last call", "last decode" and
 * zz_ctx_last_decode_members_stats state alone. */
#define ZZ_MEMBERS_FIND_LIMIT_DEFAULT (1ull << 20)   /* derived, not tuned: the tail limit of the point finder (1 MiB of compressed bytes) -- members of logs, WARC records and 64 KiB blocks end far in front of it, so round 2 is the exception */
int zz_members_find_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, uint64_t limit_bytes,
                           uint64_t* d_index, uint64_t max_entries,
                           uint64_t* entries, void* hip_stream);
/* zz_decode_members_device for files whose members announce no length: for EVERY input the return value, *out_len and the bytes
 * are what zi_members defines, that is, what zz_decode_members_device returns; only the speed differs. The members are found as
 * zz_members_find_device finds them (default limit), then:
 *   a broken walk          the serial path decides on the whole file
 *   a clean walk           the members in front of m* -- the first whose bytes pass `cap` -- are decoded as a batch, one wavefront
 *                          each, into exactly their measured lengths. If all succeed and there is no m*: ZZ_OK, *out_len = L.
 *                          Otherwise the serial path runs from the first member that did not succeed, or from m*, over what is
 *                          left of source, destination and room; the members in front of it are proven, and its answer is the
 *                          call's. A damaged or oversized file is so refused after one member's serial work, not the file's.
 * Verdicts, ZZ_E_ARG rules, *out_len = ~0 on failure and "nothing is written outside d_dst[0, cap)" are zz_decode_members_device's.
 * Workspace: zz_members_find_device's and 44 bytes per member. Synchronous. Leaves the context's "last call", "last decode" and
 * zz_ctx_last_decode_members_stats state alone. */
int zz_decode_members_found_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, void* d_dst, uint64_t cap,
                                   uint64_t* out_len, void* hip_stream);
/* what the last zz_members_find_device or zz_decode_members_found_device did: the members the walk accepted (all of them behind
 * a clean walk), the candidates, the candidates the walk stepped over, and the rounds of measures (1 or 2; all 0: no call yet, or
 * refused before anything ran) */
int zz_ctx_last_members_find_stats(const zz_ctx* ctx, uint64_t* members, uint64_t* candidates, uint64_t* dropped, uint32_t* rounds);

/* Points INSIDE members: one index over the members of any file of gzip members and the blocks inside them, the
 * cuts a decode of a file of few large members -- `cat lane1.fq.gz lane2.fq.gz`, rotated logs joined with cat -- needs to use many
 * wavefronts per member (that decode is zz_decode_members_points_device, below). The
 * result is defined by the file F, chunk_bytes C and spacing alone; bits count from F's first byte:
 *   header candidates  zz_members_find_device's: offset 0, and every offset i >= 20 where a gzip header stands with ten bytes
 *                      left behind it
 *   block candidates   zz_points_index_device's with D = F: for every chunk c >= 1 the lowest bit where a non-final dynamic block
 *                      header stands that a decoder would accept, no bit of it behind F
 *   jobs               one per candidate, measured WITHOUT WRITING A BYTE: a header job parses its header and counts from the
 *                      member's first block bit, a block job from its bit, to the first block boundary at or behind the lowest
 *                      block candidate above its first bit, or through a final block -- whose member's ISIZE it then reads
 *   walk               from offset 0: a header candidate whose job succeeded opens a member; a block boundary that is a block
 *                      candidate continues it with that candidate's job (an inner row), any other with a repair job; a job that
 *                      ends with a final block closes the member, whose ISIZE must equal the low 32 bits of its count, and the
 *                      next member begins behind its trailer -- at src_len the walk is done. Candidates the walk steps over are
 *                      dropped; a block candidate that is a member's first block bit is neither a row nor dropped.
 * The index is `entries` rows (in_bit, out_byte) in HOST memory. Member j contributes a START row (the bit of its first block |
 * ZZ_MP_START, the decoded bytes in front of it), its inner rows (bit, decoded bytes in front of the bit), and an END row (the bit
 * behind its final block | ZZ_MP_END, the decoded bytes in front of member j + 1); the last row's out_byte is L = *out_len.
 * spacing > 1 thins inner rows only, by zz_points_index_host's rule on file-absolute decoded positions, starting again at every
 * START row. *entries and *out_len are set even when max_entries is too small: the call then returns ZZ_E_NOSPACE and writes
 * nothing (2 * (src_len / 20 + 1) + src_len / chunk_bytes rows always suffice).
 *   ZZ_OK is not a verdict on CRC-32 or match distances: no byte is produced (zz_decode_members_device gives the verdict).
 *   ZZ_E_DATA: the walk breaks -- src_len == 0, a job of the walk in error, an ISIZE mismatch, a byte behind a trailer that is no
 *     header, truncation.
 *   ZZ_E_UNSUPPORTED: more than 2^31 - 1 candidates of either kind.
 *   ZZ_E_ARG, before anything is launched: a null context, entries or out_len, a null d_src with src_len > 0, null points with
 *     max_entries > 0, chunk_bytes < 16, spacing < 1, src_len >= 2^61, an unfinished zz_encode_device_async on the context.
 * Synchronous; the host reads 40 bytes per job and round and walks them. Leaves the context's "last call", "last decode" and the
 * other calls' stats alone. */
#define ZZ_MP_START (1ull << 63)
#define ZZ_MP_END (1ull << 62)
int zz_members_points_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, uint64_t chunk_bytes, uint64_t spacing,
                             uint64_t* points, uint64_t max_entries, uint64_t* entries, uint64_t* out_len, void* hip_stream);
/* what the last zz_members_points_device did: the members the walk accepted, the candidates of either kind, the candidates the
 * walk stepped over, and the rounds of jobs (all 0: no call yet, or refused before anything ran) */
int zz_ctx_last_members_points_stats(const zz_ctx* ctx, uint64_t* members, uint64_t* header_candidates, uint64_t* block_candidates,
                                     uint64_t* dropped, uint32_t* rounds);
/* Host only: the START / END rows of a member point index as zz_members_find_device's pairs (file offset, decoded offset), members
 * + 1 of them, so that zz_decode_members_ranges_device reads such files too (`index` in host memory: copy it to the device).
 * Size protocol as above. ZZ_E_DATA: the rows are not START, inner rows, END per member. */
int zz_members_points_to_index(const uint64_t* points, uint64_t entries, uint64_t* index, uint64_t max_entries, uint64_t* index_entries);
/* zz_decode_members_device for files of LARGE members, through a member point index: many wavefronts per member. For EVERY input
 * -- every file, every row array (true, thinned, lying, another file's), every cap and batch_bytes -- the return value, *out_len,
 * the bytes d_dst[0, *out_len) and "nothing is written outside d_dst[0, cap)" are what zi_members defines, that is, what
 * zz_decode_members_device gives. The index decides speed, never the result.
 *   points, entries  zz_members_points_device's rows in HOST memory (as zz_decode_points_device takes its rows). NULL with 0: the
 *                    call makes the index itself (ZZ_POINTS_CHUNK_DEFAULT, spacing 1); if that fails for any reason but ZZ_E_HIP
 *                    the serial path decides on the whole file.
 *   batch_bytes      the most decoded bytes in a batch (zz_points_windows_device's stage_bytes knob); 0 means 64 MiB.
 * The rows are an index if they are START, inner rows, END per member; their masked bits ascend strictly; every START bit is a
 * multiple of 8; out_byte ascends from 0 and every END's equals the next START's; and with c_0 = 0, c_{j+1} = ((end_j + 7) >> 3) + 8:
 * c_j + 10 <= start_j / 8 and the last c is src_len. Anything else sends the whole file to the serial path. Member j is DEALT if it
 * lies in front of m*, the first member whose END out_byte passes cap or that holds a segment longer than batch_bytes. A dealt member
 * is PROVEN iff (1) the gzip header at c_j ends exactly at start_j / 8; (2) every segment of it decodes from its bit to exactly the
 * next row's bit into exactly its room, the final block in its last segment and nowhere else, no distance reaching in front of the
 * member's first byte; (3) the CRC-32 of its bytes is the trailer's; (4) ISIZE is the low 32 bits of its length. With f the first
 * dealt member that is not proven, or m*: without f the result is ZZ_OK and *out_len = L; otherwise the serial path runs from member
 * f over what is left of source, destination and room, and its answer is the call's (DESIGN.md 23 has the argument).
 *   ZZ_E_ARG, before anything is launched: zz_decode_members_found_device's rules; null points with entries > 0; entries == 1;
 *     batch_bytes above 64 MiB.
 * *out_len = ~0 on failure. Workspace: a batch's (4 bytes and a bit per decoded byte of it), 53 bytes per segment and 65 per member.
 * Synchronous; the host reads a fixed number of words per batch and per call. Leaves the context's "last call", "last decode" and
 * the other calls' stats alone (zz_ctx_last_members_points_stats too when the call makes its own index). */
int zz_decode_members_points_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, void* d_dst, uint64_t cap,
                                    uint64_t* out_len, const uint64_t* points, uint64_t entries,
                                    uint64_t batch_bytes, void* hip_stream);
/* what the last zz_decode_members_points_device did: the members the rows name (0: the rows were no index, or none could be made),
 * the members proven in front of the serial tail (all of them: no tail), the segments dealt, the batches launched, the pending bytes
 * and the most rounds of a batch, and 1 if the serial path ran (all 0: no call yet, or refused before anything ran) */
int zz_ctx_last_decode_members_points_stats(const zz_ctx* ctx, uint64_t* members, uint64_t* proven, uint64_t* segments,
                                            uint32_t* batches, uint64_t* pending_bytes, uint32_t* rounds, int* serial);

/* Many reads of one blocked gzip (BGZF) file through its index in one call: read r receives the decoded bytes
 * [d_firsts[r], d_firsts[r] + d_nbytes[r]) of the file d_src[0, src_len). d_index / entries are an index as above (from
 * zz_members_index_device, from zz_encode_members_device's offsets, or from a .gzi file); the six arrays of nranges entries live
 * in DEVICE memory (d_status may be NULL). With c_j, u_j the index's pairs and L = u_(entries - 1): d_out_lens[r] = m =
 * min(nbytes, L - first), 0 with ZZ_OK for first == L or nbytes == 0; nothing is written outside d_dsts[r][0, min(m, cap)).
 * A read whose status is not ZZ_OK has d_out_lens[r] = ~0 and the first min(m, cap) bytes of its destination are unspecified;
 * it leaves every other read complete.
 * CHECKED COMPLETELY: every byte a read returns comes from a member that was decoded whole and accepted exactly as
 * zz_decode_batch_device accepts a gzip item -- header, blocks, CRC-32 and ISIZE, no byte behind the trailer -- and that holds
 * exactly the u_(j+1) - u_j bytes (its ROOM) the index gives it. The index is never trusted: it proposes the cuts.
 *   A member is TOUCHED by a read when it holds at least one byte of [first, first + m); empty members are never touched, and
 *     reads with ZZ_E_ARG or ZZ_E_NOSPACE touch nothing. A touched member is decoded whole and judged whole -- the price of the
 *     checksum -- and once per call, however many reads touch it.
 *   d_status[r]: ZZ_OK; ZZ_E_ARG: first > L, or first + nbytes overflows; ZZ_E_NOSPACE: m > cap; ZZ_E_DATA: a member the read
 *     touches is not what the index says -- decoding d_src[c_j, c_(j+1)) as one gzip member into u_(j+1) - u_j bytes of room
 *     does not succeed with exactly that many bytes (header, blocks, truncation, CRC-32, ISIZE, bytes behind the trailer, a room
 *     too small or too large); ZZ_E_UNSUPPORTED: no touched member is like that, but one has a room above 64 MiB (the stage).
 *   Returns ZZ_OK when every read is ZZ_OK; otherwise ZZ_E_DATA if any read is, else ZZ_E_UNSUPPORTED, else ZZ_E_ARG, else
 *     ZZ_E_NOSPACE (zz_decode_ranges_device's precedence).
 *   ZZ_E_ARG, before anything is launched: a null context, source, index, d_firsts, d_nbytes, d_dsts, d_caps or d_out_lens;
 *     entries < 2; entries - 1 or nranges above 2^31 - 1; an unfinished zz_encode_device_async on the context. nranges == 0 with
 *     arguments that pass returns ZZ_OK at once.
 *   Failure of the call as a whole, decided on the device: the index is not an index unless u_0 == 0, c ascends strictly, u
 *     ascends and the last file offset is at most src_len. Then every d_status[r] = ZZ_E_DATA, every d_out_lens[r] = ~0, no
 *     destination byte is written and the call returns ZZ_E_DATA.
 * Reads may overlap each other; destinations that overlap are the caller's error.
 * How: one thread per entry checks the index; one thread per read plans it (two binary searches, a +1 / -1 pair in
 * a difference array over the members); a scan over the members gives the touched members, their slots on a stage and their
 * waves (64 MiB of rooms each); per wave zz_decode_batch_device's kernel decodes the touched members into the stage, and the part
 * of each read that lies in the wave -- one interval of the stage -- is copied out in 64 KiB chunks dealt over the workgroups.
 * The host reads a fixed number of words for the plan, two per wave once, and two per wave's decode, whatever nranges and the
 * member count are. A single small read costs one member's decode by ONE wavefront.
 * Workspace: the stage, sized by the call's largest wave (below 128 MiB); 28 bytes per member; 44 bytes per touched member of the
 * largest wave; 32 bytes per read; 16 bytes per wave. Synchronous. Leaves the context's "last call", "last decode",
 * zz_ctx_last_decode_ranges_stats and zz_ctx_last_decode_members_stats state alone. */
int zz_decode_members_ranges_device(zz_ctx* ctx, const void* d_src, uint64_t src_len,
                                    const uint64_t* d_index, uint64_t entries,
                                    uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                    void* const* d_dsts, const uint64_t* d_caps,
                                    uint64_t* d_out_lens, int32_t* d_status, void* hip_stream);
/* what the last zz_decode_members_ranges_device did: the members it decoded (each once), and the waves */
int zz_ctx_last_decode_members_ranges_stats(const zz_ctx* ctx, uint64_t* members_decoded, uint32_t* waves);

/* ---- reads of any stream through a point index: windows and sums beside the index -----------------------------------------
 * zz_decode_points_device decodes a foreign stream only whole. To read a little out of a lot -- random access into an ordinary
 * .gz -- a segment must decode alone, and for that the index gets a SIDECAR of two arrays, for segments = entries - 1:
 *   windows  `segments` slots of ZZ_POINTS_WINDOW (32,768) bytes. Slot k holds the decoded bytes
 *            [max(0, out_byte[k] - 32768), out_byte[k]), right-aligned: the byte at distance d in front of segment k is
 *            slot[32768 - d]. The bytes in front of them in the slot are unspecified and never read; slot 0 is entirely
 *            unspecified. Slots have a fixed size so that a slot's place needs no second index.
 *   sums     `segments` little-endian uint32: entry k is the public checksum of segment k's decoded bytes, as a packet's entry
 *            of zz_packet_checksums_device: adler32 with start value 1 for zlib, crc32 for gzip and raw; an empty segment has 1 or 0.
 * 32,772 bytes per segment: 3.1 % of the decoded size at a spacing of 1 MiB, 25 % at 128 KiB. That is the trade: a read costs one
 * segment's decode by one wavefront, which grows with the spacing, and the sidecar shrinks with it.
 *
 * zz_points_windows_host makes both arrays: one more sequential pass over src[0, src_len) in HOST memory, no GPU, no context,
 * for an index from zz_points_index_host or from elsewhere. The index is verified on the way: ZZ_E_DATA unless every row's in_bit
 * is a block boundary reached with exactly its out_byte in front of it, the last row is the stream's end and length, and header and
 * trailer pass as zz_points_index_host checks them. ZZ_E_UNSUPPORTED for a preset dictionary; ZZ_E_ARG for a null pointer,
 * entries < 2 or a format outside 0..2. windows: segments * 32768 bytes, sums: segments words, both the caller's. */
#define ZZ_POINTS_WINDOW 32768u
int zz_points_windows_host(const uint8_t* src, uint64_t src_len, int format, const uint64_t* points, uint64_t entries,
                           uint8_t* windows, uint32_t* sums);

/* Many reads of one zlib / gzip / raw stream through its point index and sidecar in one call: read r receives the decoded bytes
 * [d_firsts[r], d_firsts[r] + d_nbytes[r]) of the stream d_src[0, src_len). Index (entries rows), windows and sums live in DEVICE
 * memory -- made once, read many times -- and so do the six arrays of nranges entries (d_status may be NULL). Reads, lengths,
 * statuses, the return value and its precedence are zz_decode_members_ranges_device's, with L = the last out_byte and a SEGMENT
 * where that call says member: m = min(nbytes, L - first); ZZ_E_ARG first > L or overflow; ZZ_E_NOSPACE m > cap; ZZ_E_DATA a
 * touched segment is not what index and sidecar say; ZZ_E_UNSUPPORTED none is like that, but one has a room above 64 MiB. A read
 * whose status is not ZZ_OK has d_out_lens[r] = ~0 and leaves every other read complete. A touched segment is decoded whole and
 * once per call, however many reads touch it: the price of the checksum.
 * NOTHING BESIDE THE STREAM IS TRUSTED. A segment is what index and sidecar say iff it begins at a block header, ends at the next
 *   row's bit, produces exactly its room, holds the final block iff it is the last one, no distance in it reaches in front of the
 *   stream (whatever a slot's unspecified bytes hold), and the checksum of the bytes it produced equals d_sums[k]. For zlib and
 *   gzip the sums, folded in segment order over the lengths the index gives, must give the stream's own trailer -- so a wrong
 *   window shows as a checksum mismatch, not as wrong bytes. A raw stream has no trailer: there the sums are the caller's own
 *   witness, as the sidecar of zz_decode_range_checked_device is for a raw stream.
 *   Failure of the call as a whole, decided on the device (every d_status[r] = ZZ_E_DATA, every d_out_lens[r] = ~0, no destination
 *   byte written, the call returns ZZ_E_DATA): the rows are not an index (row 0 == (0, 0), in_bit strictly ascending, out_byte
 *   ascending); the last in_bit does not end exactly where the trailer begins; the container header is invalid (a preset
 *   dictionary: the call returns ZZ_E_UNSUPPORTED); the sums do not fold to the trailer (Adler-32; CRC-32 and ISIZE against L mod
 *   2^32; lengths are 64-bit in the fold); an entry that no segment of its length can have.
 *   ZZ_E_ARG, before anything is launched: a null context, source, index, windows, sums, d_firsts, d_nbytes, d_dsts, d_caps or
 *   d_out_lens; entries < 2; entries - 1 or nranges above 2^31 - 1; a format outside 0..2; an unfinished zz_encode_device_async.
 *   nranges == 0 with arguments that pass returns ZZ_OK at once.
 * There is no serial path: errors come at the parallel rate. How: check, plan, touched scan, waves, cut, copy and
 * verdict are zz_decode_members_ranges_device's kernels called with the rows; one workgroup reads the header and folds the sums;
 * per wave one wavefront per touched segment decodes it onto the stage against its window slot, read where it lies, and sums it.
 * Workspace: the stage (below 128 MiB); 28 bytes per segment; 20 bytes per touched segment of the largest wave; 32 bytes per read;
 * 16 bytes per wave. Synchronous; the host reads a fixed number of words per call and per wave. Leaves the context's "last call",
 * "last decode", zz_ctx_last_decode_ranges_stats and zz_ctx_last_decode_members_ranges_stats state alone. */
int zz_decode_points_ranges_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format,
                                   const uint64_t* d_points, uint64_t entries, const void* d_windows, const uint32_t* d_sums,
                                   uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                   void* const* d_dsts, const uint64_t* d_caps,
                                   uint64_t* d_out_lens, int32_t* d_status, void* hip_stream);
/* what the last zz_decode_points_ranges_device did: the segments it decoded (each once), and the waves */
int zz_ctx_last_decode_points_ranges_stats(const zz_ctx* ctx, uint64_t* segments_decoded, uint32_t* waves);

/* ---- the same sidecar built on the device ----------------------------------------------------------------------
 * For a stream d_src[0, src_len) in DEVICE memory and the rows `points` (HOST memory, `entries` of them), d_windows and d_sums
 * (DEVICE: (entries - 1) * 32768 bytes, entries - 1 words) receive exactly what zz_points_windows_host makes for those rows; the
 * bytes that format leaves unspecified -- the front of a slot where the stream is shorter than 32 KiB there, all of slot 0 -- are
 * written as zeros. The stream is decoded in batches of at most stage_bytes decoded bytes (0: 64 MiB, also the most) by
 * zz_decode_points_device's kernels onto a stage of 32768 + stage_bytes bytes, and slots and sums are cut out of each batch; no
 * destination of the stream's length is needed. With d_dst (cap bytes, DEVICE) the batches decode there instead and the decoded
 * stream is left in d_dst[0, last out_byte).
 * fine_points (HOST, may be NULL): rows to DECODE with, a superset of `points` -- every row of `points` occurs in it with the same
 *   two numbers, first and last rows equal. The sidecar wants sparse rows (32,772 bytes per segment), the decode dense ones (a
 *   wavefront per segment): take the index dense (zz_points_index_device, spacing 1), thin it for the sidecar (zz_points_thin), and
 *   pass both.
 * NOTHING IS TRUSTED, and nothing is repaired: ZZ_E_DATA wherever zz_points_windows_host gives it -- rows that are not an index
 *   (row 0 == (0, 0), in_bit strictly ascending, out_byte ascending), a last row that is not the end of the final block directly in
 *   front of the trailer, a segment (of the rows decoded with) that does not begin at a block header, end at the next row's bit with
 *   exactly its room or keep its distances inside the stream, and, for zlib and gzip, sums whose fold over the 64-bit segment
 *   lengths misses the trailer (gzip: ISIZE against L mod 2^32 too). A raw stream has no trailer to hold the sums to.
 *   ZZ_E_UNSUPPORTED: a preset dictionary; a segment of the rows decoded with that is longer than the stage.
 *   After a failure the contents of d_windows, d_sums and d_dst are unspecified; nothing is written outside them.
 * ZZ_E_ARG, before anything is launched: a null context, source, points, d_windows or d_sums; entries < 2; entries - 1 above
 *   2^31 - 1; a format outside 0..2; stage_bytes above 64 MiB; d_dst null with cap > 0; fine_points that is no superset of points;
 *   an unfinished zz_encode_device_async. ZZ_E_NOSPACE, nothing written: d_dst given and cap below the last out_byte.
 * Workspace: the stage, 4 bytes of pointer and 1 bit per byte of a batch, 32 bytes per segment of a batch. Synchronous; the host
 * reads the batch's counters and its sums (4 bytes per segment) once per batch and folds them. Leaves the context's "last call",
 * "last decode" path and stats and the range calls' stats alone. */
int zz_points_windows_device(zz_ctx* ctx, const void* d_src, uint64_t src_len, int format,
                             const uint64_t* points, uint64_t entries, const uint64_t* fine_points, uint64_t fine_entries,
                             void* d_windows, uint32_t* d_sums, void* d_dst, uint64_t cap, uint64_t stage_bytes, void* hip_stream);
/* what the last zz_points_windows_device did: decode batches launched, the bytes phase 1 left pending, the most rounds of a batch */
int zz_ctx_last_points_windows_stats(const zz_ctx* ctx, uint64_t* batches, uint64_t* pending_bytes, uint32_t* rounds);
/* An index thinned on the host by the builders' own rule: row 0 and the last row stay, an inner row stays iff it is the first at
 * or behind the next multiple of `spacing` decoded bytes -- zz_points_thin(index at spacing 1, s) is the index at spacing s.
 * *out_entries is set whenever the arguments pass (ZZ_E_NOSPACE: max_entries is too small, or out is NULL). ZZ_E_ARG: a null
 * points or out_entries, entries < 2, spacing 0. */
int zz_points_thin(const uint64_t* points, uint64_t entries, uint64_t spacing, uint64_t* out, uint64_t max_entries, uint64_t* out_entries);

enum { ZZ_DECODE_INDEXED = 1, ZZ_DECODE_DISCOVERED = 2, ZZ_DECODE_SERIAL = 3, ZZ_DECODE_POINTS = 4 };
/* which path the last zz_decode_device / zz_decode_points_device finished on (0: none) */
int zz_ctx_last_decode_path(const zz_ctx* ctx);
/* the packet index the last zz_decode_device recovered by discovery (path ZZ_DECODE_DISCOVERED; ZZ_E_ARG otherwise), in
 * the form of zz_packet_index_device: *entries = packets + 1 (set even when max_entries is too small: ZZ_E_NOSPACE) */
int zz_ctx_last_decode_index_device(zz_ctx* ctx, uint64_t* d_index, uint64_t max_entries, uint64_t* entries, void* hip_stream);
/* what the last zz_decode_device's or zz_decode_points_device's parallel path saw: bytes phase 1 left pending (their match
 * source lay in front of their packet or segment) and the pointer-jumping rounds that resolved them (0 and 0 on the serial path) */
int zz_ctx_last_decode_stats(const zz_ctx* ctx, uint64_t* pending_bytes, uint32_t* rounds);

/* container pieces for assembling shards on the host */
int zz_header(int format, uint8_t out[10]);                                   /* returns 0/2/10 */
int zz_trailer(int format, uint32_t cks_total, uint64_t n, uint8_t out[8]);   /* returns 0/4/8  */

/* ---- checksums (host utilities, adler.cpp / crc.cpp semantics) ------------------------------------- */
uint32_t zz_adler32(uint32_t start, const uint8_t* p, uint64_t n);
uint32_t zz_adler32_combine(uint32_t first, uint32_t second_start0, uint64_t len_second);
uint32_t zz_crc32(const uint8_t* p, uint64_t n, uint32_t start);
uint32_t zz_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* ---- synthetic inputs (BASELINE.json configs), generated on the device ------------------------------ */
enum { ZZ_GEN_TEXT = 0, ZZ_GEN_RANDOM = 1, ZZ_GEN_LOG = 2, ZZ_GEN_MIX = 3 };
/* fills d_buf[0,n); byte i is a pure function of (kind, seed, first_byte + i), in 64 KiB blocks (first_byte must
 * be a multiple of 65536) */
int zz_generate_device(zz_ctx* ctx, int kind, uint64_t seed, uint64_t first_byte, void* d_buf, uint64_t n,
                       void* hip_stream);
/* the same bytes computed on the host (for parity sampling) */
int zz_generate_host(int kind, uint64_t seed, uint64_t first_byte, uint8_t* buf, uint64_t n);

const char* zz_last_error(void);
const char* zz_version(void);
/* the compile-time experiment switches this binary carries, space-separated; "" for the product build (some of them write
 * deliberately wrong streams for timing runs: a deployment can assert on "") */
const char* zz_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif
