// zz_api.hip -- host side of libzzflate_amd.so: contexts, workspaces, kernel launches and the C ABI
// declared in include/zzflate_amd.h. Mirrors the L4 layer of the reference (zzflate.cpp): container
// header, range split, fan-out, in-order join, trailer -- with the fan-out being "packets -> wavefronts".
//
// There is no CPU encode path in this library: every byte of DEFLATE output is produced by the HIP
// kernels, and every entry point fails with ZZ_E_HIP when no device is usable.
#include <hip/hip_runtime.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/zzflate_amd.h"
#include "zz_common.h"
#include "zz_wave.h"
#include "zz_checksum.h"
#include "zz_emit.h"
#include "zz_level0.h"
#include "zz_level1.h"
#include "zz_level1p.h"
#include "zz_level2.h"
#include "zz_stream2.h"
#include "zz_compact.h"
#include "zz_datagen.h"
#include "zz_verify.h"
#include "zz_inflate.h"
#include "zz_inflate_ranges.h"
#include "zz_inflate_check.h"
#include "zz_inflate_points.h"
#include "zz_inflate_points_find.h"
#include "zz_inflate_members.h"
#include "zz_inflate_members_find.h"
#include "zz_inflate_members_points.h"
#include "zz_inflate_members_decode.h"
#include "zz_inflate_members_ranges.h"
#include "zz_inflate_points_ranges.h"
#include "zz_inflate_points_windows.h"
#include "zz_batch.h"
#include "zz_members_write.h"

using namespace zz;

static thread_local std::string g_err;
static void set_err(const std::string& s) { g_err = s; }
extern "C" const char* zz_last_error(void) { return g_err.c_str(); }
extern "C" const char* zz_version(void) { return "zzflate_amd 0.1 (gfx950)"; }
// Compile-time switches this binary was built with that change what it computes or records, as a space-separated list; "" for the
// product build. ZZ_PROF adds cycle stamps (tools/prof_l1p.py, tools/prof_phases.py); ZZ_ST_ALWAYS_CAREFUL is the test build
// libzzflate_amd_careful.so. tests/test_abi.py holds the shipped library to "".
extern "C" const char* zz_build_flags(void)
{
    return ""
#ifdef ZZ_PROF
        " ZZ_PROF"
#endif
#ifdef ZZ_ST_ALWAYS_CAREFUL
        " ZZ_ST_ALWAYS_CAREFUL"
#endif
        ;
}

#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            set_err(std::string(#expr) + ": " + hipGetErrorString(_e));                  \
            return ZZ_E_HIP;                                                             \
        }                                                                                \
    } while (0)

// The one owner of a context's device memory (zz_buf<T>) and pinned host memory (zz_pin<T>): `cap` elements at `p`, freed when the
// context is deleted -- a buffer added to zz_ctx needs no line anywhere else. grow() keeps what is large enough; otherwise it frees
// first and allocates then (the peak stays at one buffer, and hipFree waits for the device), and cap is set only on success.
template <class T, bool PINNED = false> struct zz_buf {
    T* p = nullptr;
    uint64_t cap = 0;
    zz_buf() = default;
    zz_buf(const zz_buf&) = delete;
    zz_buf& operator=(const zz_buf&) = delete;
    ~zz_buf() { release(); }
    void release()
    {
        if (PINNED) (void)hipHostFree(p); else (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    int grow(uint64_t count)
    {
        if (count <= cap) return ZZ_OK;
        release();
        if (PINNED) HIPCHK(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault));
        else HIPCHK(hipMalloc((void**)&p, count * sizeof(T)));
        cap = count;
        return ZZ_OK;
    }
    uint64_t bytes() const { return cap * sizeof(T); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};
template <class T> using zz_pin = zz_buf<T, true>;

struct zz_ctx {
    int device = 0;
    // workspace (grown on demand, kept across calls so steady-state calls do not allocate)
    zz_buf<uint8_t> slots;
    zz_buf<uint32_t> sizes; zz_buf<uint64_t> offsets; zz_buf<zz_cks> cks;      // per packet: grown together (ensure_workspace)
    zz_buf<uint8_t> l2_scratch;
    zz_buf<zz_result> d_res; zz_buf<zz_cks_total> d_cks_total;
    zz_buf<uint32_t> d_err;              // 4 words; what they mean: read_err_word
    zz_pin<zz_result> h_res;
    zz_buf<unsigned long long> d_prof;   // 64 counters for diagnostic (-DZZ_PROF) builds
    zz_buf<uint8_t> d_tail;              // 128 bytes: the end of the shard being encoded, then zeros (k_encode_l1p's over-reads)
    // staging for the host-buffer entry points
    zz_buf<uint8_t> stage_in, stage_out;
    // slab pipeline of the host-buffer entry points: pinned slabs in and out, device output slabs, three streams
    zz_pin<uint8_t> pin_in[2], pin_out[2];
    zz_buf<uint8_t> slab_out[2];
    zz_buf<uint8_t> slab_in[2];          // device input ring: halo + slab each
    hipStream_t s_in = nullptr, s_enc = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = { nullptr, nullptr }, ev_out[2] = { nullptr, nullptr };
    // what the last packet-mode call did, for zz_verify_last_device
    zz_verify_params last = {};  bool have_last = false;
    bool idx_empty = false; uint64_t idx_empty_bytes = 0;   // the last packet-mode call had an empty input (zz_packet_index_device)
    zz_buf<unsigned long long> d_verify;
    // zz_encode_batch_device: per item (first packet, slot base, tail: ensure_items), per packet (descriptor), the plan's totals
    struct {
        zz_buf<uint32_t> first; zz_buf<uint64_t> slotbase; zz_buf<uint8_t> tails;     // (tails: 128 bytes per item)
        zz_buf<zz_batch_desc> desc;
        zz_buf<zz_batch_totals> d_tot; zz_pin<zz_batch_totals> h_tot;
    } bat;
    // zz_encode_members_device: per member (source, length; file offset (+1 entry), stored flag), what the host reads, the last call's stats
    struct {
        zz_buf<const uint8_t*> srcs; zz_buf<uint64_t> ns, moff; zz_buf<uint8_t> stored;
        zz_buf<zz_mw_state> d_st; zz_pin<zz_mw_state> h_st;
        uint64_t members = 0, stored_members = 0;
    } mw;
    zz_buf<uint32_t> d_work;             // level 2: packet counter of the persistent workgroups
    zz_buf<uint64_t> d_log;              // sequential stream, callback form: EnsureOutputLength log, two words per entry
    // a call that has been enqueued but not waited for (zz_encode_device_async .. zz_encode_finish)
    struct {
        bool active = false; hipStream_t st = nullptr; uint32_t npk = 0; int level = 0; bool whole = false;
        // the call itself, for the rerun behind a run-time LDS-order violation (encode_finish)
        bool order_checked = false;          // the launch relied on the LDS's lane order and checked it in the kernel
        const uint8_t* d_src = nullptr; uint64_t n = 0, halo = 0; bool last_is_final = false; uint8_t* d_dst = nullptr; uint64_t cap = 0;
        int format = 0, cks_kind = 0, level_asked = 0; uint32_t P = 0; uint32_t warm = 0;
    } pend;
    zz_pin<uint32_t> h_err;              // the kernels' sticky error word
    uint32_t warm = 0;                   // levels >= 1: warm window in bytes (0 = cold packets, the reference's threaded mode)
    bool extended = false;               // levels 4..6 accepted (beyond the reference)
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_time = false;
    // decode (zz_decode_device): one batch of phase-1 / phase-2 workspace, per-packet results of the call, discovery's candidates
    struct {
        zz_buf<uint32_t> st;                                  // pointers, 4 bytes per output byte of a batch
        zz_buf<uint32_t> pend;                                // bitmap words
        zz_buf<uint32_t> pcnt, prem;
        zz_buf<uint64_t> ends; zz_buf<uint32_t> stat;
        zz_buf<uint64_t> cand;                                // candidates, then a recovered index
        zz_buf<zz_cks> cks;
        zz_buf<unsigned long long> tot;                       // 64 counters (zz_inf_params::tot)
        zz_buf<zz_inf_serial_out> sres; zz_buf<uint32_t> ok;
        zz_buf<unsigned long long> items_ctr;                 // zz_decode_batch_device: [0..1] failure counters, [2] the dealing counter
        zz_pin<unsigned long long> items_host;                // the two failure counters
        int last_path = 0; uint64_t last_pending = 0; uint32_t last_rounds = 0;
        // zz_decode_range_device: the carried bytes and one batch (ZI_BIAS + B * P), the carried bytes' external bits, its stats
        zz_buf<uint8_t> stage; zz_buf<uint32_t> xcarry;
        struct { uint64_t first_packet = 0, packets = 0, pending = 0; uint32_t attempts = 0; } range;
        // zz_decode_ranges_device: per read its record, per stage packet of a wave its descriptor, what the host reads per attempt
        zz_buf<zi_read> rng_reads; zz_buf<zi_read_desc> rng_desc;
        zz_buf<zz_rng_totals> rng_tot; zz_pin<zz_rng_totals> rng_host;
        struct { uint64_t packets = 0, retried = 0; uint32_t attempts = 0, waves = 0; } ranges;
        // the checked reads and zz_packet_checksums_device (zz_inflate_check.h): per packet of the stream a partial (the sidecar unpacked,
        // or the producer's sums), per stage packet its sum, the sidecar's fold, the verdict words
        zz_buf<zz_cks> side, scks; zz_buf<zz_cks_total> side_total; zz_buf<uint32_t> verdict;
        std::vector<uint64_t> last_index;                     // the index discovery recovered (zz_ctx_last_decode_index_device)
        // zz_decode_points_device (zz_inflate_points.h): a batch's rows, its segments' results, the dealing counter
        struct { zz_buf<uint64_t> rows; zz_buf<zz_pt_stat> stat; zz_buf<unsigned int> next; } pts;
        // zz_points_index_device (zz_inflate_points_find.h): one record per chunk (the candidates, then a round's jobs and their
        // results in place), the dealing counter, and what the last call did
        struct {
            zz_buf<zi_find_job> job; zz_buf<unsigned int> next;
            uint64_t candidates = 0, dropped = 0; uint32_t rounds = 0;
        } pf;
        // zz_decode_members_device: per stretch of the mark pass (count, base), per candidate (offset, length; then the member
        // list), per member k_inflate_items' descriptors, what the host reads, the serial path's result
        struct {
            zz_buf<uint32_t> blk_cnt; zz_buf<uint64_t> blk_base;
            zz_buf<uint64_t> offs; zz_buf<uint32_t> lens;
            zz_buf<const uint8_t*> srcs; zz_buf<uint8_t*> dsts; zz_buf<uint64_t> src_lens, caps, out_lens;
            zz_buf<zz_mem_state> st; zz_pin<zz_mem_state> h_st;
            zz_buf<zz_inf_members_out> sres; zz_pin<zz_inf_members_out> h_sres;
            uint64_t members = 0, candidates = 0; int path = 0;
        } mem;
        // zz_members_find_device, zz_decode_members_found_device (zz_inflate_members_find.h): per candidate its record, its flag
        // and (round 2) its number, the dealing counter, the dealt members' statuses, what the host reads behind the slots, and what
        // the last call did; the mark pass's buffers, the descriptors and the serial path's result are mem's
        struct {
            zz_buf<zi_find_job> rec; zz_buf<uint8_t> keep; zz_buf<uint32_t> which; zz_buf<unsigned int> next;
            zz_buf<int32_t> status;
            zz_buf<zz_mf_state> st; zz_pin<zz_mf_state> h_st;
            uint64_t members = 0, candidates = 0, dropped = 0; uint32_t rounds = 0;
        } mf;
        // zz_members_points_device (zz_inflate_members_points.h): the block candidates, a round's jobs (results in place), the dealing
        // counter, and what the last call did. The mark passes' buffers are mem's and pf's
        struct {
            zz_buf<uint64_t> bc; zz_buf<zi_mp_job> job; zz_buf<unsigned int> next;
            uint64_t members_found = 0, header_candidates = 0, block_candidates = 0, dropped = 0; uint32_t rounds = 0;
        } mp;
        // zz_decode_members_points_device (zz_inflate_members_decode.h): the dealt descriptors and members of the call, per descriptor
        // its flag and its sum, per member its status, the verdict's word, the dealing counter, and what the last call did. The batch's
        // workspace is dec_points_workspace's, the serial path's result is mem's
        struct {
            zz_buf<zi_mpd_seg> seg; zz_buf<zi_mpd_member> mem; zz_buf<uint8_t> segok, status; zz_buf<uint32_t> sums;
            zz_buf<unsigned long long> first_bad; zz_buf<unsigned int> next;
            uint64_t members = 0, proven = 0, segments = 0, pending = 0; uint32_t batches = 0, rounds = 0; int serial = 0;
        } mpd;
        // the reads through an index (dec_reads; zz_inflate_members_ranges.h): the stage, per read (record, chunk scan), per unit
        // (differences, counts), per touched unit (list, S, F, G), per unit of a wave its status, per wave two words, what the
        // host reads; a wave's rooms and lengths (and k_inflate_items' descriptors) are mem's
        struct {
            zz_buf<uint8_t> stage;
            zz_buf<zi_mr_read> reads; zz_buf<uint64_t> chunk0;
            zz_buf<int32_t> diff; zz_buf<uint32_t> cnt, tlist, F, G; zz_buf<uint64_t> S;
            zz_buf<int32_t> status;
            zz_buf<uint64_t> waves; zz_pin<uint64_t> h_waves;
            zz_buf<zz_mr_state> st; zz_pin<zz_mr_state> h_st;
        } rd;
        // what the last zz_decode_members_ranges_device did
        struct { uint64_t decoded = 0; uint32_t waves_run = 0; } mr;
        // zz_decode_points_ranges_device (zz_inflate_points_ranges.h): what its front leaves, and what the last call did
        struct {
            zz_buf<zz_pr_state> st; zz_pin<zz_pr_state> h_st;
            uint64_t decoded = 0; uint32_t waves_run = 0;
        } pr;
        // zz_points_windows_device (zz_inflate_points_windows.h): the stage (32 KiB carried, then a batch), the rows the cut works on,
        // two slots nobody keeps and one sum (a sidecar segment longer than the stage is cut piece by piece), the dealing counter,
        // and what the last call did
        struct {
            zz_buf<uint8_t> stage, spare; zz_buf<uint64_t> rows; zz_buf<uint32_t> piece; zz_buf<unsigned int> next;
            uint64_t batches = 0, pending = 0; uint32_t rounds = 0;
        } pw;
    } dec;
};
// one call per context at a time: every entry point that would use the buffers of an enqueued call refuses
static bool call_pending(const zz_ctx* c)
{
    if (c->pend.active) set_err("a call enqueued with zz_encode_device_async has not been finished on this context");
    return c->pend.active;
}

// Small host values (an empty input's block, a result record whose size is known up front) reach the device as kernel
// ARGUMENTS -- copied at launch -- not as asynchronous copies from stack locals, which would still be read after an
// enqueue-only call (zz_encode_device_async) has returned.
// the last min(n, 64) bytes of a shard, then zeros: what k_encode_l1p reads instead of bytes past the shard's end
__global__ void k_fill_tail(const uint8_t* src, uint64_t n, uint8_t* tail)
{
    const uint64_t tn = n < 64 ? n : 64;
    const uint32_t i = threadIdx.x;
    tail[i] = i < tn ? src[n - tn + i] : (uint8_t)0;
}
__global__ void k_put_small(uint8_t* dst, uint64_t bytes, uint32_t nbytes, zz_result* res, uint64_t stream_bytes)
{
    for (uint32_t i = 0; i < nbytes; ++i) dst[i] = (uint8_t)(bytes >> (8 * i));
    if (res) res->stream_bytes = stream_bytes;
}

static int header_len(int format) { return format == ZZ_ZLIB ? 2 : format == ZZ_GZIP ? 10 : 0; }
static int trailer_len(int format) { return format == ZZ_ZLIB ? 4 : format == ZZ_GZIP ? 8 : 0; }

// worst-case bytes one packet can occupy in its slot, per level (multiple of 16)
static uint32_t slot_stride_for(int level, uint32_t P) { return zz_slot_stride(level, P); }

extern "C" uint64_t zz_bound(uint64_t n, int format, int level, uint32_t P)
{
    if (P == 0 || P > ZZ_MAX_PACKET_SIZE) P = ZZ_DEFAULT_PACKET;
    uint64_t npk = n ? (n + P - 1) / P : 1;
    uint64_t per;
    if (level == 0) per = (uint64_t)P + 10;
    else if (level == 1) per = ((uint64_t)9 * P + 10 + 7) / 8 + 6;
    else per = (uint64_t)P + 11;
    return header_len(format) + npk * per + trailer_len(format) + 16;
}

static bool lds_order_ok(int device);
extern "C" int zz_ctx_create(int device, zz_ctx** out)
{
    if (!out) { set_err("null out"); return ZZ_E_ARG; }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        set_err(std::string("no HIP device available (hipGetDeviceCount: ") + hipGetErrorString(e) + ", count " +
                std::to_string(count) + "): this library has no CPU encode path");
        return ZZ_E_HIP;
    }
    if (device < 0 || device >= count) { set_err("bad device index"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(device));
    zz_ctx* c = new zz_ctx();
    c->device = device;
    const int rc = [&]() -> int {
        if (int rc = c->d_res.grow(1)) return rc;
        if (int rc = c->d_cks_total.grow(1)) return rc;
        if (int rc = c->d_err.grow(4)) return rc;
        if (int rc = c->d_work.grow(16)) return rc;
        if (int rc = c->d_prof.grow(64)) return rc;
        if (int rc = c->d_tail.grow(128)) return rc;
        HIPCHK(hipMemset(c->d_prof, 0, 64 * sizeof(unsigned long long)));
        if (int rc = c->h_res.grow(1)) return rc;
        if (int rc = c->h_err.grow(4)) return rc;
        HIPCHK(hipEventCreate(&c->ev0));
        HIPCHK(hipEventCreate(&c->ev1));
        (void)lds_order_ok(device);          // the probe, once per device, HERE: the launch sites only read its cached verdict
        return ZZ_OK;
    }();
    if (rc) { zz_ctx_destroy(c); return rc; }                            // nothing allocated so far is left behind
    *out = c;
    return ZZ_OK;
}

extern "C" void zz_ctx_destroy(zz_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->pend.active) { (void)hipStreamSynchronize(c->pend.st); c->pend.active = false; }   // an enqueued call still uses the buffers
    for (int i = 0; i < 2; ++i) {
        if (c->ev_in[i]) (void)hipEventDestroy(c->ev_in[i]);
        if (c->ev_out[i]) (void)hipEventDestroy(c->ev_out[i]);
    }
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_enc) (void)hipStreamDestroy(c->s_enc);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;                            // frees every buffer (zz_buf)
}

extern "C" uint64_t zz_ctx_workspace_bytes(const zz_ctx* c)
{
    if (!c) return 0;
    return c->slots.bytes() + c->sizes.bytes() + c->offsets.bytes() + c->cks.bytes() + c->l2_scratch.bytes() + c->stage_in.bytes() +
           c->stage_out.bytes() + c->bat.first.bytes() + c->bat.slotbase.bytes() + c->bat.tails.bytes() + c->bat.desc.bytes() +
           c->mw.srcs.bytes() + c->mw.ns.bytes() + c->mw.moff.bytes() + c->mw.stored.bytes();
}
// diagnostic (not part of the public header): workgroups of the level's encode kernel the runtime places on one CU
extern "C" int zz_debug_occupancy(int level)
{
    int nb = -1;
    if (level == 1) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_encode_l1p, ZZ_L1P_THREADS, 0);
    else if (level == -1) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_encode_l1, ZZ_L1_THREADS, 0);
    else if (level >= 4) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_encode_l2_t<32768u, true>, ZZ_L2_THREADS, 0);
    else if (level >= 2) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_encode_l2_t<0u, false, true>, ZZ_L2P_THREADS, 0);
    else if (level == -2) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_encode_l2_t<0u, false>, ZZ_L2_THREADS, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_encode_l0, 256, 0);
    return nb;
}
// diagnostic (not part of the public header): does the LDS serve the lanes of one wavefront instruction that add to one
// address in ascending lane order, and one wavefront's instructions in issue order? k_l6_matches' counting sort takes its places
// from exactly that (zz_level6.h). Runs `trials` pairs of 64-key blocks per wavefront in 16-wavefront workgroups on every CU, keys
// drawn with many duplicates (shared dwords, shared banks, one heavy key, all equal ...); *bad = the number of returned counts
// that differ from the lane-ascending, block-ascending ones (0 on gfx950).
__global__ __launch_bounds__(1024) void k_lds_order_probe(uint32_t seed, uint32_t trials, unsigned long long* bad)
{
    __shared__ uint32_t T[16][256];                // 512 packed 16-bit counters per wavefront
    __shared__ uint16_t K[16][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = lane; i < 256; i += 64) T[wave][i] = 0;
    uint32_t x = seed ^ (blockIdx.x * 2654435761u) ^ (threadIdx.x * 40503u);
    unsigned long long nbad = 0;
    for (uint32_t t = 0; t < trials; ++t) {
        uint32_t k[2];
        for (int u = 0; u < 2; ++u) {
            x = x * 1664525u + 1013904223u;
            const uint32_t r = x >> 8;
            switch ((t + blockIdx.x) & 7u) {
            case 0: k[u] = r % 512u; break;                          // few duplicates
            case 1: k[u] = r % 16u; break;                           // many
            case 2: k[u] = r % 3u; break;                            // three values, two of them in one dword
            case 3: k[u] = 7u; break;                                // all the same
            case 4: k[u] = (r % 8u) * 64u; break;                    // one bank, different addresses
            case 5: k[u] = (r % 4u) * 64u + ((r >> 5) & 1u); break;  // one bank, halves of a dword
            case 6: k[u] = (lane & 1) ? 5u : r % 512u; break;        // one heavy key among light ones
            default: k[u] = r % 40u; break;
            }
            K[wave][u * 64 + lane] = (uint16_t)k[u];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // two blocks back to back, no wait between them
        const uint32_t oa = atomicAdd(&T[wave][k[0] >> 1], 1u << ((k[0] & 1u) << 4));
        const uint32_t ob = atomicAdd(&T[wave][k[1] >> 1], 1u << ((k[1] & 1u) << 4));
        const uint32_t ra = (oa >> ((k[0] & 1u) << 4)) & 0xFFFFu, rb = (ob >> ((k[1] & 1u) << 4)) & 0xFFFFu;
        uint32_t wa = 0, wb = 0;                                     // what lane order gives
        for (int i = 0; i < 64; ++i) {
            if (i < lane && K[wave][i] == k[0]) ++wa;
            if (K[wave][i] == k[1]) ++wb;                            // all of block A come first ...
            if (i < lane && K[wave][64 + i] == k[1]) ++wb;           // ... then the lower lanes of block B
        }
        if (ra != wa) ++nbad;
        if (rb != wb) ++nbad;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        atomicSub(&T[wave][k[0] >> 1], 1u << ((k[0] & 1u) << 4));
        atomicSub(&T[wave][k[1] >> 1], 1u << ((k[1] & 1u) << 4));
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // the same for the masked exchange the level-1 and level-2 parsers insert with (zz_level1.h): every lane puts lane + 1 into
        // its key's 16-bit half and must get back what the nearest lower lane with that key put there (0: none); afterwards the
        // half holds the highest lane's; and a non-returning one under a lane mask leaves the highest masked lane's
        {
            const uint32_t sh = (k[0] & 1u) << 4;
            const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)&T[wave][k[0] >> 1];
            uint32_t old;
            asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(addr), "v"(0xFFFFu << sh), "v"((uint32_t)(lane + 1) << sh) : "memory");
            uint32_t wprev = 0, whigh = 0, wmask = 0;
            const uint64_t msk = ((uint64_t)x << 32 | (x * 2246822519u)) | (t & 1u ? 0ull : ~0ull >> (x & 63u));   // some lanes, or most
            for (int i = 0; i < 64; ++i)
                if (K[wave][i] == k[0]) {
                    if (i < lane) wprev = (uint32_t)i + 1;
                    whigh = (uint32_t)i + 1;
                    if ((msk >> i) & 1) wmask = (uint32_t)i + 65;
                }
            if (((old >> sh) & 0xFFFFu) != wprev) ++nbad;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (((T[wave][k[0] >> 1] >> sh) & 0xFFFFu) != whigh) ++nbad;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            ((uint16_t*)T[wave])[k[0]] = 0;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const uint64_t mskw = ((uint64_t)readlane((uint32_t)(msk >> 32), 0) << 32) | readlane((uint32_t)msk, 0);   // one mask for the wavefront
            uint32_t wm2 = 0;
            for (int i = 0; i < 64; ++i) if (K[wave][i] == k[0] && ((mskw >> i) & 1)) wm2 = (uint32_t)i + 65;
            (void)wmask;
            if ((mskw >> lane) & 1)
                asm volatile("ds_mskor_b32 %0, %1, %2" :: "v"(addr), "v"(0xFFFFu << sh), "v"((uint32_t)(lane + 65) << sh) : "memory");
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (((T[wave][k[0] >> 1] >> sh) & 0xFFFFu) != wm2) ++nbad;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            ((uint16_t*)T[wave])[k[0]] = 0;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            // plain 16-bit stores: two blocks back to back; the slot must end up with the LAST store's highest lane (the warm
            // window's pre-hash enters its positions with nothing else: zz_level1.h warm_prehash)
            ((uint16_t*)T[wave])[k[0]] = (uint16_t)(lane + 1);
            ((uint16_t*)T[wave])[k[1]] = (uint16_t)(lane + 65);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            uint32_t ws = 0;
            for (int i = 0; i < 64; ++i) if (K[wave][i] == k[0]) ws = (uint32_t)i + 1;
            for (int i = 0; i < 64; ++i) if (K[wave][64 + i] == k[0]) ws = (uint32_t)i + 65;
            if (((uint16_t*)T[wave])[k[0]] != ws) ++nbad;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            ((uint16_t*)T[wave])[k[0]] = 0;
            ((uint16_t*)T[wave])[k[1]] = 0;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
    }
    if (nbad) atomicAdd(bad, nbad);
}
extern "C" int zz_debug_lds_atomic_order(zz_ctx* c, uint32_t trials, unsigned long long* bad, unsigned long long* checked)
{
    if (!c || !bad) return ZZ_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(unsigned long long)));
    HIPCHK(hipMemset(d, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_lds_order_probe, dim3(512), dim3(1024), 0, 0, 0x5EEDu, trials, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(bad, d, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipFree(d));
    if (checked) *checked = 512ull * 1024ull * 6ull * trials;
    return ZZ_OK;
}
// diagnostic (not part of the public header): the code construction of levels 2..6 on histograms of the caller's (k_debug_code_lengths,
// zz_level2.h). All pointers are host memory. Case c: desc[4c] = mode (0: the frequency-floor limiter calc_lengths_w, 1: package-merge
// pm_lengths_w), desc[4c + 1] = n (286 / 30 / 19), desc[4c + 2] = maxlen (15 / 15 / 7: the pairs the packet kernels use), freqs[288c ..
// 288c + n). Out: lens[288c ..], codes[288c ..] = (len << 16) | bits, and for n = 286 / 30 recs[320c ..] = value | payload << 8,
// meta[20c .. 20c + 19) the meta frequencies, meta[20c + 19] the record count. The limiter's heap keeps a count and a tree index in
// one word (count << 10 | index, the root's count included: sums below 2^22) and package-merge sorts on count << 9 | symbol and adds
// weights in 32 bits; a packet's counts sum to at most 32,769. The hook admits sums up to 2^20, a margin below the first of those
// bounds and far above a packet: ZZ_E_ARG otherwise.
extern "C" int zz_debug_code_lengths(zz_ctx* c, uint32_t ncases, const uint32_t* desc, const uint32_t* freqs, uint8_t* lens, uint32_t* codes,
                                     uint16_t* recs, uint32_t* meta)
{
    if (!c || !desc || !freqs || !lens || !codes || !recs || !meta) { set_err("null argument"); return ZZ_E_ARG; }
    if (ncases == 0) return ZZ_OK;
    if (ncases > 65536u) { set_err("too many cases"); return ZZ_E_ARG; }
    for (uint32_t k = 0; k < ncases; ++k) {
        const uint32_t mode = desc[4 * k], n = desc[4 * k + 1], maxlen = desc[4 * k + 2];
        uint64_t sum = 0;
        if (mode > 1 || !((n == 286 && maxlen == 15) || (n == 30 && maxlen == 15) || (n == 19 && maxlen == 7))) { set_err("bad case descriptor"); return ZZ_E_ARG; }
        for (uint32_t i = 0; i < n; ++i) sum += freqs[288ull * k + i];
        if (sum > (1u << 20)) { set_err("counts of a case sum to more than 2^20"); return ZZ_E_ARG; }
    }
    HIPCHK(hipSetDevice(c->device));
    zz_buf<uint32_t> d_desc, d_freqs, d_codes, d_meta;
    zz_buf<uint8_t> d_lens;
    zz_buf<uint16_t> d_recs;
    int rc;
    if ((rc = d_desc.grow(4ull * ncases)) || (rc = d_freqs.grow(288ull * ncases)) || (rc = d_codes.grow(288ull * ncases)) ||
        (rc = d_meta.grow(20ull * ncases)) || (rc = d_lens.grow(288ull * ncases)) || (rc = d_recs.grow(320ull * ncases))) return rc;
    HIPCHK(hipMemcpy(d_desc, desc, 4ull * ncases * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_freqs, freqs, 288ull * ncases * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_lens, 0, 288ull * ncases));
    HIPCHK(hipMemset(d_codes, 0, 288ull * ncases * sizeof(uint32_t)));
    HIPCHK(hipMemset(d_recs, 0, 320ull * ncases * sizeof(uint16_t)));
    HIPCHK(hipMemset(d_meta, 0, 20ull * ncases * sizeof(uint32_t)));
    zz_dbg_cl_params q; q.desc = d_desc; q.freqs = d_freqs; q.lens = d_lens; q.codes = d_codes; q.recs = d_recs; q.meta = d_meta;
    hipLaunchKernelGGL(k_debug_code_lengths, dim3(ncases), dim3(ZZ_WAVE), 0, 0, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(lens, d_lens, 288ull * ncases, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(codes, d_codes, 288ull * ncases * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(recs, d_recs, 320ull * ncases * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(meta, d_meta, 20ull * ncases * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ZZ_OK;
}
// diagnostic (not part of the public header): the planning kernels' workgroup scan alone (wg_scan_excl, wg_scan_excl2: zz_wave.h),
// as they use it -- one workgroup of `threads` (256 or 1024), one value per thread and round, a carry from round to round, the
// round's closing barrier. All pointers are host memory. form 0: n uint32_t, form 1: n uint64_t, form 2: n pairs { a, b } of
// uint64_t scanned together, a in 32 bits (its upper half is ignored and comes back zero), b in 64. out[i] = the sum of in[0 .. i)
// in the form's width (32-bit sums wrap), total = the sum of all; out and total have in's layout.
template <int THREADS, class V> __global__ __launch_bounds__(THREADS) void k_debug_wg_scan(const V* in, uint64_t n, V* out, V* total)
{
    __shared__ V wtot[THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    V carry = 0;
    for (uint64_t r0 = 0; r0 < n; r0 += THREADS) {
        const uint64_t i = r0 + t;
        const wg_prefix<V> s = wg_scan_excl<THREADS>(i < n ? in[i] : (V)0, wtot);
        if (i < n) out[i] = carry + s.excl;
        carry += s.total;
        __syncthreads();
    }
    if (t == 0) *total = carry;
}
template <int THREADS> __global__ __launch_bounds__(THREADS) void k_debug_wg_scan2(const uint64_t* in, uint64_t n, uint64_t* out, uint64_t* total)
{
    __shared__ uint32_t wa[THREADS / ZZ_WAVE];
    __shared__ uint64_t wb[THREADS / ZZ_WAVE];
    const uint32_t t = threadIdx.x;
    uint32_t ca = 0; uint64_t cb = 0;
    for (uint64_t r0 = 0; r0 < n; r0 += THREADS) {
        const uint64_t i = r0 + t;
        const uint32_t a = i < n ? (uint32_t)in[2 * i] : 0;
        const uint64_t b = i < n ? in[2 * i + 1] : 0;
        const wg_prefix2<uint32_t, uint64_t> s = wg_scan_excl2<THREADS>(a, wa, b, wb);
        if (i < n) { out[2 * i] = ca + s.a.excl; out[2 * i + 1] = cb + s.b.excl; }
        ca += s.a.total; cb += s.b.total;
        __syncthreads();
    }
    if (t == 0) { total[0] = ca; total[1] = cb; }
}
extern "C" int zz_debug_wg_scan(zz_ctx* c, int form, uint32_t threads, uint64_t n, const void* in, void* out, void* total)
{
    if (!c || !total || (n && (!in || !out))) { set_err("null argument"); return ZZ_E_ARG; }
    if (form < 0 || form > 2 || (threads != 256 && threads != 1024) || n > (1ull << 24)) { set_err("bad form, threads or n"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const uint64_t words = form == 0 ? (n + 1) / 2 : form == 1 ? n : 2 * n;       // of 8 bytes; the last 32-bit value may share one
    const uint64_t bytes = (form == 0 ? 4 : form == 1 ? 8 : 16) * n, tbytes = form == 0 ? 4 : form == 1 ? 8 : 16;
    zz_buf<uint64_t> d_in, d_out, d_total;
    int rc;
    if ((rc = d_in.grow(words + 1)) || (rc = d_out.grow(words + 1)) || (rc = d_total.grow(2))) return rc;
    if (n) HIPCHK(hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0xFF, (words + 1) * sizeof(uint64_t)));
    HIPCHK(hipMemset(d_total, 0xFF, 2 * sizeof(uint64_t)));
    const bool big = threads == 1024;
    if (form == 0) {
        if (big) hipLaunchKernelGGL((k_debug_wg_scan<1024, uint32_t>), dim3(1), dim3(1024), 0, 0, (const uint32_t*)d_in.p, n, (uint32_t*)d_out.p, (uint32_t*)d_total.p);
        else hipLaunchKernelGGL((k_debug_wg_scan<256, uint32_t>), dim3(1), dim3(256), 0, 0, (const uint32_t*)d_in.p, n, (uint32_t*)d_out.p, (uint32_t*)d_total.p);
    } else if (form == 1) {
        if (big) hipLaunchKernelGGL((k_debug_wg_scan<1024, uint64_t>), dim3(1), dim3(1024), 0, 0, (const uint64_t*)d_in.p, n, d_out.p, d_total.p);
        else hipLaunchKernelGGL((k_debug_wg_scan<256, uint64_t>), dim3(1), dim3(256), 0, 0, (const uint64_t*)d_in.p, n, d_out.p, d_total.p);
    } else {
        if (big) hipLaunchKernelGGL((k_debug_wg_scan2<1024>), dim3(1), dim3(1024), 0, 0, (const uint64_t*)d_in.p, n, d_out.p, d_total.p);
        else hipLaunchKernelGGL((k_debug_wg_scan2<256>), dim3(1), dim3(256), 0, 0, (const uint64_t*)d_in.p, n, d_out.p, d_total.p);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(total, d_total, tbytes, hipMemcpyDeviceToHost));
    return ZZ_OK;
}
// ---- the run-time guard for that property ---------------------------------------------------------------------------------
// Three things in this library are only correct where the LDS serves equal addresses of one instruction in ascending lane order
// and one wavefront's instructions in issue order -- which gfx950 does and its ISA manual does not promise: the warm window's
// pre-hash (zz_level1.h warm_prehash), the extended levels' counting sort (zz_level6.h) and the two-wavefront level-1 kernel
// (zz_level1p.h: a slot ends up with the HIGHEST lane's store). So the probe above runs once per device, the first time one of
// them is asked for, and its verdict is kept: where it fails, zz_ctx_set_warm_window(> 0) and zz_ctx_set_extended_levels(1) are
// refused with ZZ_E_UNSUPPORTED and level 1 runs its one-wavefront kernel (k_encode_l1, which asks the LDS for nothing of the
// kind); levels 0..3 with cold packets never depend on it. zz_debug_force_lds_order lets a test take the refusal path.
static std::mutex g_order_mu;
static std::atomic<int> g_order_verdict[64];     // per device: 0 unknown, 1 holds, -1 does not
static std::atomic<int> g_order_forced{-1};      // -1: probe; 0 / 1: the verdict every device gets (tests)
static std::atomic<int> g_force_violation{0};    // tests: the next level-1 / warm-window launches report a violated order (bit 4 of the error word)
extern "C" void zz_debug_force_lds_order(int verdict) { g_order_forced.store(verdict < 0 ? -1 : (verdict ? 1 : 0)); }
// (not part of the public header) n > 0: the next n encode launches that check the order in the kernel (k_encode_l1p, the warm window's
// pre-hash) behave as if they had seen it violated -- the test of the rerun / refusal path behind that check
extern "C" void zz_debug_force_lds_violation(int launches) { g_force_violation.store(launches < 0 ? 0 : launches); }
// (not part of the public header) forget a device's verdict (tests put back what a forced violation flipped)
extern "C" void zz_debug_reset_lds_order(int device) { if (device >= 0 && device < 64) g_order_verdict[device].store(0); }
// Runs the probe where the device has no verdict yet. Blocking (allocation, a kernel on the null stream, a synchronous copy): called
// from zz_ctx_create and the setters, never from an enqueue-only entry point -- the launch sites read the cached verdict
// (lds_order_cached: one atomic load, no HIP call, nothing that would break a stream capture or sit between two timing events).
static bool lds_order_ok(int device)
{
    const int forced = g_order_forced.load();
    if (forced >= 0) return forced == 1;
    if (device < 0 || device >= 64) return false;
    if (g_order_verdict[device].load() == 0) {
        std::lock_guard<std::mutex> lk(g_order_mu);
        if (g_order_verdict[device].load() == 0) {
            unsigned long long bad = 1, *d = nullptr;
            int prev = 0;
            bool ran = hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess && hipMalloc(&d, sizeof(bad)) == hipSuccess;
            if (ran) {
                ran = hipMemset(d, 0, sizeof(bad)) == hipSuccess;
                if (ran) {
                    hipLaunchKernelGGL(k_lds_order_probe, dim3(512), dim3(1024), 0, 0, 0xC0FFEEu ^ (uint32_t)device, 4u, d);   // 12.6 M checks, < 1 ms
                    ran = hipGetLastError() == hipSuccess && hipMemcpy(&bad, d, sizeof(bad), hipMemcpyDeviceToHost) == hipSuccess;
                }
                (void)hipFree(d);
                (void)hipSetDevice(prev);
            }
            if (!ran) (void)hipGetLastError();
            g_order_verdict[device].store((ran && bad == 0) ? 1 : -1);
        }
    }
    return g_order_verdict[device].load() == 1;
}
// the verdict as the launch sites read it: every context's creation has run the probe for its device
static inline bool lds_order_cached(int device)
{
    const int forced = g_order_forced.load(std::memory_order_relaxed);
    if (forced >= 0) return forced == 1;
    return device >= 0 && device < 64 && g_order_verdict[device].load(std::memory_order_relaxed) == 1;
}
// A kernel saw the order violated at run time (bit 4 of the error word: zz_level1p.h P2, zz_level1.h warm_prehash): the device loses
// its verdict for the rest of the process -- level 1 runs k_encode_l1 from here on, warm windows and extended levels are refused.
static void lds_order_revoke(int device) { if (device >= 0 && device < 64) g_order_verdict[device].store(-1); }
// (not part of the public header) the verdict for a device: 1 holds, 0 does not
extern "C" int zz_debug_lds_order_verdict(int device) { return lds_order_ok(device) ? 1 : 0; }
// diagnostic builds only (not part of the public header): read and clear the per-phase cycle counters
extern "C" int zz_debug_read_prof(zz_ctx* c, unsigned long long out[16])
{
    if (!c) return ZZ_E_ARG;
    HIPCHK(hipMemcpy(out, c->d_prof, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(c->d_prof, 0, 16 * sizeof(unsigned long long)));
    return ZZ_OK;
}
// the same for kernels that keep one set of 16 counters per wavefront of the workgroup (k_encode_l1p: set w = wavefront w)
extern "C" int zz_debug_read_prof_sets(zz_ctx* c, unsigned long long out[64])
{
    if (!c) return ZZ_E_ARG;
    HIPCHK(hipMemcpy(out, c->d_prof, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(c->d_prof, 0, 64 * sizeof(unsigned long long)));
    return ZZ_OK;
}
// warm window. At level 1 the last `bytes` bytes (at most 32768) in front of every packet -- as far as
// they exist in the stream: a shard must pass them as its halo -- are hashed into the packet's table before it is parsed,
// so that matches may reach back across the packet boundary. 0 (the default) gives the reference's threaded stream.
extern "C" int zz_ctx_set_warm_window(zz_ctx* c, uint32_t bytes)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (bytes > 32768) { set_err("warm window must be 0..32768 bytes"); return ZZ_E_ARG; }
    if (bytes && !lds_order_ok(c->device)) {
        set_err("warm window refused: this device's LDS does not serve equal addresses in lane order (probe k_lds_order_probe failed)");
        return ZZ_E_UNSUPPORTED;
    }
    c->warm = bytes;
    return ZZ_OK;
}
// levels beyond the reference. Off by default, so that the entry points keep the reference's error
// convention for level > 3; on: levels 4, 5, 6 = chains of depth 2 / 4 / 8, lazy matching, package-merge (zz_level6.h).
extern "C" int zz_ctx_set_extended_levels(zz_ctx* c, int on)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (on && !lds_order_ok(c->device)) {
        set_err("extended levels refused: this device's LDS does not serve equal addresses in lane order (probe k_lds_order_probe failed)");
        return ZZ_E_UNSUPPORTED;
    }
    c->extended = on != 0;
    return ZZ_OK;
}
extern "C" void zz_ctx_enable_timing(zz_ctx* c, int on) { if (c) { c->timing = on != 0; c->have_time = false; } }
extern "C" double zz_ctx_last_kernel_ms(zz_ctx* c)
{
    if (!c || !c->timing || !c->have_time) return -1.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0;
    return ms;
}

static int ensure_workspace(zz_ctx* c, int level, uint64_t npk, uint32_t stride, int xdepth = 0, uint32_t P = 0)
{
    if (npk > c->cks.cap) {              // (the last of the three: a failure half way leaves it empty, and the next call starts over)
        c->sizes.release(); c->offsets.release(); c->cks.release();
        if (int rc = c->sizes.grow(npk)) return rc;
        if (int rc = c->offsets.grow(npk)) return rc;
        if (int rc = c->cks.grow(npk)) return rc;
    }
    if (level != 0) if (int rc = c->slots.grow(npk * stride)) return rc;
    if (level >= 2) if (int rc = c->l2_scratch.grow(l2_scratch_bytes((uint32_t)npk, xdepth, P))) return rc;
    return ZZ_OK;
}
// batches and members, per item: first packet and slot base (`items_plus_one` entries), tail (128 bytes each) -- grown together
static int ensure_items(zz_ctx* c, uint64_t items_plus_one)
{
    if (items_plus_one * 128 <= c->bat.tails.cap) return ZZ_OK;    // (the last of the three, as in ensure_workspace)
    c->bat.first.release(); c->bat.slotbase.release(); c->bat.tails.release();
    if (int rc = c->bat.first.grow(items_plus_one)) return rc;
    if (int rc = c->bat.slotbase.grow(items_plus_one)) return rc;
    return c->bat.tails.grow(items_plus_one * 128);
}
// batches and members, per packet: sizes, offsets and checksum partials, the items' slots end to end (slot_bytes == 0: none),
// level 2's scratch (xdepth: with the extended levels' words and chains), the descriptors
static int ensure_batch_workspace(zz_ctx* c, int level, uint32_t npk, uint64_t slot_bytes, uint32_t P, int xdepth)
{
    if (int rc = ensure_workspace(c, 0, npk, 0)) return rc;
    if (int rc = c->slots.grow(slot_bytes)) return rc;
    if (level >= 2) if (int rc = c->l2_scratch.grow(l2_scratch_bytes(npk, xdepth, P))) return rc;
    return c->bat.desc.grow(npk);
}
// staging of the host-buffer entry points and of zz_encode_multi_device's pulls (64 bytes of room behind what was asked for)
static int ensure_stage(zz_ctx* c, uint64_t in_bytes, uint64_t out_bytes)
{
    if (in_bytes > c->stage_in.cap) if (int rc = c->stage_in.grow(in_bytes + 64)) return rc;
    if (out_bytes > c->stage_out.cap) if (int rc = c->stage_out.grow(out_bytes + 64)) return rc;
    return ZZ_OK;
}

// ZZFLATE_L1_KERNEL=classic (diagnostic, A/B): one parsing wavefront per packet (k_encode_l1) instead of the two of k_encode_l1p;
// the streams are the same
static bool l1_classic()
{
    static const bool classic = [] { const char* e = getenv("ZZFLATE_L1_KERNEL"); return e && !strcmp(e, "classic"); }();
    return classic;
}
// ZZFLATE_L2_KERNEL=classic (diagnostic, A/B): one parsing wavefront per packet at levels 2,3 instead of two; the streams are the same
static bool l2_classic()
{
    static const bool classic = [] { const char* e = getenv("ZZFLATE_L2_KERNEL"); return e && !strcmp(e, "classic"); }();
    return classic;
}
// Which kernel form a packet-mode launch takes -- the one place that decides it, for single calls, batches (warm = 0, xdepth = 0) and the
// zz_debug_l?_kernel queries. l1p: level 1 on k_encode_l1p (two parsing wavefronts) instead of k_encode_l1; l2p: levels 2,3 on
// k_encode_l2p (its insert is an ordered exchange: zz_level2p.h) instead of k_encode_l2_t<0, false>; both want cold packets,
// a positive LDS-order verdict and no ZZFLATE_L?_KERNEL=classic, and one_parser (the rerun behind a violation) rules them out.
// order_checked: the launch relies on the LDS's lane order and checks it as it goes (error value 4): those two, and the warm window's pre-hash.
// (The extended levels, a batch's or a member file's too, come as level 2 with their window and xdepth: neither form, no check.)
struct launch_plan { bool l1p, l2p, order_checked; };
static launch_plan plan_launch(const zz_ctx* c, int level, uint32_t warm, int xdepth, bool one_parser)
{
    launch_plan p;
    p.l1p = level == 1 && !warm && !one_parser && !l1_classic() && lds_order_cached(c->device);
    p.l2p = level >= 2 && !warm && xdepth == 0 && !one_parser && !l2_classic() && lds_order_cached(c->device);
    p.order_checked = p.l1p || (warm != 0 && xdepth == 0) || p.l2p;
    return p;
}
// tests (zz_debug_force_lds_violation): one of the launches that were to report a violated order is this one
static bool take_forced_violation()
{
    int left = g_force_violation.load();
    while (left > 0 && !g_force_violation.compare_exchange_weak(left, left - 1)) {}
    return left > 0;
}
// The packet kernels' sticky error word (zz_packet_params::err = d_err[0]; the sequential stream also keeps "truncated" in d_err[1] and
// its log's entries in d_err[2]), read from h_err[0] once the call's stream has been waited for:
//   value 4 (ZZ_ERR_LDS_ORDER): a kernel saw the LDS leave a LOWER lane's store in a slot that a higher lane of the same instruction wrote
//     too (zz_level1p.h P2; zz_level1.h warm_prehash; zz_level2p.h's exchange). What it wrote is a valid stream, but not necessarily the
//     reference's: the device loses its verdict and the caller runs the call again on the one-parser kernels (ERR_RERUN), which ask the
//     LDS for nothing of the kind (same bytes where the two-parser ones are right);
//   anything else (ZZ_ERR_SLOT_OVERFLOW): a packet did not fit its slot.
enum { ERR_RERUN = 1 };              // (the ZZ_E_* codes are negative)
static int read_err_word(zz_ctx* c, bool order_checked)
{
    const uint32_t e = c->h_err[0];
    if (e & 4u) {
        lds_order_revoke(c->device);
        if (!order_checked) { set_err("internal: LDS-order violation reported by a kernel that does not check it"); return ZZ_E_HIP; }
        return ERR_RERUN;
    }
    if (e) { set_err("internal: packet slot overflow"); return ZZ_E_NOSPACE; }
    return ZZ_OK;
}
// (not part of the public header) which level-1 kernel a cold packet-mode call on this context would launch now: 2 = k_encode_l1p
// (two parsing wavefronts), 1 = k_encode_l1 (ZZFLATE_L1_KERNEL=classic, or the device's LDS-order verdict is negative)
extern "C" int zz_debug_l1_kernel(const zz_ctx* c) { return (c && plan_launch(c, 1, 0, 0, false).l1p) ? 2 : 1; }
// (the same for levels 2,3: 2 = k_encode_l2p, 1 = the two-wavefront k_encode_l2_t<0, false>)
extern "C" int zz_debug_l2_kernel(const zz_ctx* c) { return (c && plan_launch(c, 2, 0, 0, false).l2p) ? 2 : 1; }

// ---- what the encode drivers share ----------------------------------------------------------------------------------------
// Every encode call starts here: whatever zz_ctx_last_kernel_ms, zz_verify_last_device / zz_packet_extent_device and
// zz_packet_index_device could look at is about to change (they describe single packet-mode calls only).
static void begin_encode_call(zz_ctx* c) { c->have_time = false; c->have_last = false; c->idx_empty = false; }

// Checksum partials of pp's packets by pp.cks_kind (none: nothing), and their fold into d_cks_total. CRC: persistent workgroups (the table
// and the shift constants are built once per block); Adler: the grid's cap is the caller's (the packet kernels make their own Adler partials).
static void launch_cks_partials(const zz_packet_params& pp, uint32_t adler_cap, hipStream_t st)
{
    if (pp.cks_kind == ZZ_CKS_CRC) hipLaunchKernelGGL(k_crc32_packets, dim3(pp.npk < 2048 ? pp.npk : 2048), dim3(ZZ_CRC_THREADS), 0, st, pp);
    else if (pp.cks_kind == ZZ_CKS_ADLER) hipLaunchKernelGGL(k_adler_packets, dim3(pp.npk < adler_cap ? pp.npk : adler_cap), dim3(ZZ_WAVE), 0, st, pp);
}
static void launch_cks_fold(zz_ctx* c, const zz_packet_params& pp, int cks_kind, hipStream_t st)      // (pp.cks_kind may have been cleared)
{
    if (cks_kind != ZZ_CKS_NONE)
        hipLaunchKernelGGL(k_cks_reduce, dim3(1), dim3(ZZ_RED_THREADS), 0, st, pp.cks, pp.npk, pp.packet_size, pp.n, cks_kind, c->d_cks_total);
}

// What every packet-mode launch is given, as a batch's or a member file's packets take it (final, cold, slots end to end; a packet's own
// view counts its item's: zz_packet_view); a single stream adds its own. One forced violation is consumed per order-checked launch.
static zz_packet_params packet_params(zz_ctx* c, uint32_t npk, uint32_t P, int cks_kind, const launch_plan& plan)
{
    zz_packet_params pp = {};
    pp.packet_size = P; pp.npk = npk; pp.cks_kind = cks_kind; pp.last_is_final = 1;
    pp.slots = c->slots; pp.sizes = c->sizes; pp.cks = c->cks; pp.err = c->d_err; pp.prof = c->d_prof;
    pp.dbg_viol = plan.order_checked && take_forced_violation() ? 1 : 0;
    return pp;
}
// The one place that launches the packet encoders, for a single stream (M == nullptr) and for the items of a batch map. The timed work
// begins here: the CRC-32 pass of a gzip container (after it the encode kernels must not overwrite the CRC partials), then level 1's or
// levels 2..6's kernel by the plan. The level-0 forms differ between the callers and follow this call; end_packet_encoders closes it.
// (Round 3 ran the CRC pass BESIDE the encode kernel on a second stream, in front of it or behind it, with 256..2048 workgroups:
// 96.3-96.7 GB/s against 95.9 on 1 GiB of log lines at level 1, and slower at level 2 -- its LDS table lookups and VALU work come out
// of what the encode kernel's waiting parsers leave each other. Not worth a second stream: profiles/README.md.)
static int launch_packet_encoders(zz_ctx* c, zz_packet_params& pp, const zz_batch_map* M, int level, int xdepth, launch_plan plan, hipStream_t st)
{
    if (c->timing) HIPCHK(hipEventRecord(c->ev0, st));
    if (pp.cks_kind == ZZ_CKS_CRC) {
        if (M) hipLaunchKernelGGL(k_crc32_packets_batch, dim3(pp.npk < 2048 ? pp.npk : 2048), dim3(ZZ_CRC_THREADS), 0, st, pp, *M);
        else launch_cks_partials(pp, 0, st);
        pp.cks_kind = ZZ_CKS_NONE;
    }
    if (level == 0) return ZZ_OK;
    if (!M) hipLaunchKernelGGL(k_fill_tail, dim3(1), dim3(128), 0, st, pp.src, pp.n, c->d_tail);   // (what reads past the shard's end reads this)
    if (level >= 2) {
        launch_level2(pp, c->l2_scratch, c->d_work, st, xdepth, plan.l2p, M);
    } else if (M) {
        if (plan.l1p) hipLaunchKernelGGL(k_encode_l1p_batch, dim3(pp.npk), dim3(ZZ_L1P_THREADS), 0, st, pp, *M);
        else hipLaunchKernelGGL(k_encode_l1_batch, dim3(pp.npk), dim3(ZZ_L1_THREADS), 0, st, pp, *M);
    } else {
        // ZZFLATE_L1_PAD_LDS (diagnostic): extra dynamic LDS per workgroup, to measure throughput vs. resident waves
        static const unsigned pad_lds = [] { const char* e = getenv("ZZFLATE_L1_PAD_LDS"); return e ? (unsigned)atoi(e) : 0u; }();
        // (a warm window exists only where the LDS-order verdict is positive: zz_ctx_set_warm_window; k_encode_l1w = the one-parser form, A/B)
        if (pp.warm && !l1_classic()) hipLaunchKernelGGL(k_encode_l1pw, dim3(pp.npk), dim3(ZZ_L1P_THREADS), pad_lds, st, pp);
        else if (pp.warm) hipLaunchKernelGGL(k_encode_l1w, dim3(pp.npk), dim3(ZZ_L1_THREADS), pad_lds, st, pp);
        else if (!plan.l1p) hipLaunchKernelGGL(k_encode_l1, dim3(pp.npk), dim3(ZZ_L1_THREADS), pad_lds, st, pp);
        else hipLaunchKernelGGL(k_encode_l1p, dim3(pp.npk), dim3(ZZ_L1P_THREADS), pad_lds, st, pp);
    }
    return ZZ_OK;
}
// the end of the timed work, and where every packet starts in the joined stream (level 0: every packet has its known place)
static int end_packet_encoders(zz_ctx* c, int level, uint32_t npk, hipStream_t st)
{
    if (c->timing) { HIPCHK(hipEventRecord(c->ev1, st)); c->have_time = true; }
    if (level != 0) hipLaunchKernelGGL(k_scan_sizes, dim3(1), dim3(ZZ_SCAN_THREADS), 0, st, c->sizes, npk, c->offsets, c->d_res);
    return ZZ_OK;
}
// batches and members: the sticky error word behind the call's last kernel, the wait, the word's verdict (read_err_word).
// (encode_finish waits on its own: zz_encode_device_async only enqueues.)
static int finish_err_word(zz_ctx* c, bool order_checked, hipStream_t st)
{
    HIPCHK(hipMemcpyAsync(c->h_err, c->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return read_err_word(c, order_checked);
}

// The common pipeline. with_container: write header/trailer (whole stream) or not (shard).
static int encode_finish(zz_ctx* c, zz_result* host_res);
// `host_res` == nullptr: enqueue only (zz_encode_device_async); the caller collects with encode_finish.
static int encode_common(zz_ctx* c, const uint8_t* d_src, uint64_t n, uint64_t halo, bool last_is_final,
                         uint8_t* d_dst, uint64_t cap, int format, int cks_kind, bool with_container, int level,
                         uint32_t P, hipStream_t st, zz_result* host_res, bool one_parser = false)
{
    const int level_asked = level;
    if (call_pending(c)) return ZZ_E_ARG;
    begin_encode_call(c);              // a call that is refused below is still the context's last call: there is then none to look at
    // Levels 4..6 are beyond the reference (which rejects them, zzflate.cpp:201,230) and only exist when switched on:
    // hash chains of depth 2 / 4 / 8 over a window of 8 / 32 / 32 KiB in front of every packet, lazy matching, package-merge
    // code lengths (zz_level6.h), in the level-2 kernel's frame (dynamic blocks, stored fallback).
    uint32_t warm = level >= 1 ? c->warm : 0;
    int xdepth = 0;
    if (level >= 4 && level <= 6 && c->extended) {
        xdepth = level == 4 ? 2 : level == 5 ? 4 : 8;
        warm = level == 4 ? 8192u : 32768u;            // the levels bring their own window (zz_ctx_set_warm_window is for levels 1..3)
        level = 2;
    }
    if (level < 0 || level > 3) { set_err("level must be 0..3 (zzflate.cpp:201,230)"); return ZZ_E_LEVEL; }
    if (P == 0 || P > ZZ_MAX_PACKET_SIZE) { set_err("packet size must be 1..32768"); return ZZ_E_ARG; }
    if (!d_dst || (!d_src && n)) { set_err("null buffer"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const int hl = with_container ? header_len(format) : 0;
    const int tl = with_container ? trailer_len(format) : 0;
    if (cap < (uint64_t)hl) { set_err("destination smaller than the container header"); return ZZ_E_NOSPACE; }
    const uint64_t npk64 = (n + P - 1) / P;
    if (npk64 > 0x7FFFFFFFull) { set_err("too many packets for one call"); return ZZ_E_ARG; }
    const uint32_t npk = (uint32_t)npk64;
    const uint32_t stride = slot_stride_for(level, P);
    const launch_plan plan = plan_launch(c, level, warm, xdepth, one_parser);

    HIPCHK(hipMemsetAsync(c->d_res, 0, sizeof(zz_result), st));
    HIPCHK(hipMemsetAsync(c->d_cks_total, 0, sizeof(zz_cks_total), st));
    HIPCHK(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), st));

    if (npk == 0) {
        // empty input: the reference emits no block at all, which is not a valid stream;
        // emit one empty final block instead (stored at level 0, fixed otherwise)
        uint8_t blk[5]; uint32_t bl;
        if (!last_is_final) bl = 0;
        else if (level == 0) { blk[0] = 1; blk[1] = 0; blk[2] = 0; blk[3] = 0xFF; blk[4] = 0xFF; bl = 5; }
        else { blk[0] = 0x03; blk[1] = 0x00; bl = 2; }
        if ((uint64_t)hl + bl + tl > cap) { set_err("destination too small"); return ZZ_E_NOSPACE; }
        uint64_t packed = 0;
        for (uint32_t i = 0; i < bl; ++i) packed |= (uint64_t)blk[i] << (8 * i);
        hipLaunchKernelGGL(k_put_small, dim3(1), dim3(1), 0, st, d_dst + hl, packed, bl, c->d_res, (uint64_t)bl);
    } else {
        if (int rc = ensure_workspace(c, level, npk, stride, xdepth, P)) return rc;
        zz_packet_params pp = packet_params(c, npk, P, cks_kind, plan);
        pp.src = d_src; pp.n = n; pp.halo = halo; pp.last_is_final = last_is_final ? 1 : 0; pp.warm = warm; pp.slot_stride = stride; pp.tail = c->d_tail;
        if (int rc = launch_packet_encoders(c, pp, nullptr, level, xdepth, plan, st)) return rc;
        if (level == 0) {
            const uint64_t total = (uint64_t)(npk - 1) * l0_packet_bytes(P, false) +
                                   l0_packet_bytes((uint32_t)(n - (uint64_t)(npk - 1) * P), last_is_final);
            if ((uint64_t)hl + total + tl > cap) { set_err("destination too small"); return ZZ_E_NOSPACE; }
            zz_l0_params q; q.pk = pp; q.dst = d_dst + hl; q.stream_mode = 0;
            uint32_t g = npk < 16384 ? npk : 16384;
            hipLaunchKernelGGL(k_encode_l0, dim3(g), dim3(256), 0, st, q);
            hipLaunchKernelGGL(k_put_small, dim3(1), dim3(1), 0, st, (uint8_t*)nullptr, 0ull, 0u, c->d_res, total);
        }
        if (int rc = end_packet_encoders(c, level, npk, st)) return rc;
        if (level != 0) {
            uint32_t g = npk < 65536 ? npk : 65536;
            hipLaunchKernelGGL(k_compact, dim3(g), dim3(256), 0, st, c->slots, stride, c->sizes, c->offsets, npk,
                               d_dst + hl, cap >= (uint64_t)(hl + tl) ? cap - hl - tl : 0, c->d_res);
        }
        launch_cks_fold(c, pp, cks_kind, st);
    }
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1), 0, st, d_dst, cap, with_container ? format : (int)ZZ_FMT_DEFLATE,
                       c->d_cks_total, n, c->d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_res, c->d_res, sizeof(zz_result), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c->h_err, c->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (npk) {
        zz_verify_params& v = c->last;     // completed by encode_finish (stream_bytes)
        v.src = d_src; v.n = n; v.halo = halo; v.packet_size = P; v.npk = npk; v.last_is_final = last_is_final ? 1 : 0;
        v.stream = d_dst + hl; v.stream_bytes = 0;
        v.offsets = level ? c->offsets : nullptr; v.sizes = level ? c->sizes : nullptr;
        v.l0_stride = (uint32_t)l0_packet_bytes(P, false);
    }
    c->pend.active = true; c->pend.st = st; c->pend.npk = npk; c->pend.level = level; c->pend.whole = with_container;
    c->pend.order_checked = plan.order_checked;
    c->pend.d_src = d_src; c->pend.n = n; c->pend.halo = halo; c->pend.last_is_final = last_is_final; c->pend.d_dst = d_dst; c->pend.cap = cap;
    c->pend.format = format; c->pend.cks_kind = cks_kind; c->pend.level_asked = level_asked; c->pend.P = P; c->pend.warm = warm;
    if (!host_res) return ZZ_OK;
    return encode_finish(c, host_res);
}
// wait for the call encode_common enqueued on this context and collect its result
static int encode_finish(zz_ctx* c, zz_result* host_res)
{
    if (!c->pend.active) { set_err("nothing enqueued on this context"); return ZZ_E_ARG; }
    c->pend.active = false;
    HIPCHK(hipStreamSynchronize(c->pend.st));
    *host_res = *c->h_res;
    const int ew = read_err_word(c, c->pend.order_checked);
    if (ew == ERR_RERUN) {
        if (c->pend.warm) {          // a warm window has no one-parser form
            set_err("warm window: this device's LDS served equal addresses out of lane order during the call (checked in the kernel); "
                    "the stream is valid DEFLATE but not the defined one -- warm windows are refused on this device from now on");
            return ZZ_E_UNSUPPORTED;
        }
        const auto q = c->pend;
        return encode_common(c, q.d_src, q.n, q.halo, q.last_is_final, q.d_dst, q.cap, q.format, q.cks_kind, q.whole, q.level_asked, q.P,
                             q.st, host_res, true);
    }
    if (ew) return ew;
    if (host_res->err) { set_err("destination too small for the compressed stream"); return ZZ_E_NOSPACE; }
    if (c->pend.npk) { c->last.stream_bytes = host_res->stream_bytes; c->have_last = true; }
    else if (c->pend.whole || c->pend.last_is_final) { c->idx_empty = true; c->idx_empty_bytes = host_res->stream_bytes; }
    return ZZ_OK;
}

// inflate every packet of the stream the last packet-mode call on this context produced (device
// entry points; its source and destination must still be in place) and compare with that call's input.
extern "C" int zz_verify_last_device(zz_ctx* c, uint64_t* bad_packets, uint64_t* first_bad_packet, void* hip_stream)
{
    if (!c || !bad_packets) { set_err("null argument"); return ZZ_E_ARG; }
    if (!c->have_last) { set_err("no packet-mode call to verify on this context"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = c->d_verify.grow(2)) return rc;
    const unsigned long long init[2] = { 0ull, ~0ull };
    HIPCHK(hipMemcpyAsync(c->d_verify, init, sizeof init, hipMemcpyHostToDevice, st));
    zz_verify_params v = c->last;
    v.out = c->d_verify;
    hipLaunchKernelGGL(k_verify_packets, dim3((v.npk + 63) / 64), dim3(64), 0, st, v);
    HIPCHK(hipGetLastError());
    unsigned long long res[2];
    HIPCHK(hipMemcpyAsync(res, c->d_verify, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *bad_packets = res[0];
    if (first_bad_packet) *first_bad_packet = res[1];
    return ZZ_OK;
}

// Where packet k of the stream the last packet-mode call on this context produced lies: *offset counts from the first
// byte of the DEFLATE stream (behind the container header), *bytes is the packet's length. Packets are independent
// (cold table, byte-aligned: zzflate.cpp:101-125), so this is a random-access index into the stream -- and what the
// full-size tests use to compare sampled packets of a multi-GiB call with the oracle.
extern "C" int zz_packet_extent_device(zz_ctx* c, uint64_t packet, uint64_t* offset, uint64_t* bytes, void* hip_stream)
{
    if (!c || !offset || !bytes) { set_err("null argument"); return ZZ_E_ARG; }
    if (!c->have_last) { set_err("no packet-mode call on this context"); return ZZ_E_ARG; }
    const zz_verify_params& v = c->last;
    if (packet >= v.npk) { set_err("packet index out of range"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    if (!v.offsets) {                                         // level 0: every packet has its known place
        *offset = packet * v.l0_stride;
        *bytes = packet + 1 < v.npk ? v.l0_stride : v.stream_bytes - packet * v.l0_stride;
        return ZZ_OK;
    }
    uint64_t o = 0; uint32_t sz = 0;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(hipMemcpyAsync(&o, v.offsets + packet, sizeof o, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&sz, v.sizes + packet, sizeof sz, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *offset = o; *bytes = sz;
    return ZZ_OK;
}

static int cks_kind_for(int format) { return format == ZZ_ZLIB ? ZZ_CKS_ADLER : format == ZZ_GZIP ? ZZ_CKS_CRC : ZZ_CKS_NONE; }

// ---- decode (zz_inflate.h) --------------------------------------------------------------------------------------------

// The packet index of the last packet-mode call: where every packet starts behind the container header, and the stream's
// end. An empty input's one empty block counts as a packet of 0 bytes.
extern "C" int zz_packet_index_device(zz_ctx* c, uint64_t* d_index, uint64_t max_entries, uint64_t* entries, void* hip_stream)
{
    if (!c || !entries) { set_err("null argument"); return ZZ_E_ARG; }
    if (!c->have_last && !c->idx_empty) { set_err("no packet-mode call on this context"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t npk = c->have_last ? c->last.npk : 1;
    *entries = npk + 1;
    if (max_entries < npk + 1 || !d_index) { set_err("index buffer too small"); return ZZ_E_NOSPACE; }
    if (!c->have_last) {
        const uint64_t h[2] = { 0, c->idx_empty_bytes };
        HIPCHK(hipMemcpyAsync(d_index, h, sizeof h, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return ZZ_OK;
    }
    const zz_verify_params& v = c->last;
    if (!v.offsets) {                                         // level 0: every packet has its known place
        std::vector<uint64_t> h(npk + 1);
        for (uint64_t k = 0; k < npk; ++k) h[k] = k * v.l0_stride;
        h[npk] = v.stream_bytes;
        HIPCHK(hipMemcpyAsync(d_index, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(d_index, v.offsets, npk * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(d_index + npk, &v.stream_bytes, 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

extern "C" int zz_ctx_last_decode_path(const zz_ctx* c) { return c ? c->dec.last_path : 0; }
extern "C" int zz_ctx_last_decode_stats(const zz_ctx* c, uint64_t* pending_bytes, uint32_t* rounds)
{
    if (!c) { set_err("null context"); return ZZ_E_ARG; }
    if (pending_bytes) *pending_bytes = c->dec.last_pending;
    if (rounds) *rounds = c->dec.last_rounds;
    return ZZ_OK;
}

// the parallel paths' workspace (rc: what growing it gave): when it cannot be had, the sticky HIP error is cleared and the call goes
// to the serial path, which needs none
static bool dec_have(int rc) { if (rc != ZZ_OK) (void)hipGetLastError(); return rc == ZZ_OK; }

// what the parallel paths return (negative: a HIP error)
enum { DEC_SERIAL = 0,      // not taken: the index, the packet size or discovery does not fit this stream
       DEC_DONE = 1,        // decoded; *out = bytes
       DEC_NOSPACE = 2 };   // decoded -- so this is the stream's true output -- but it does not fit the destination

// ---- what the decode drivers share (a batch's geometry and its rounds: zz_inf_geometry, zz_inf_rounds in zz_inflate.h) ---------
static bool dec_format_ok(int format) { const bool ok = format >= ZZ_ZLIB && format <= ZZ_DEFLATE; if (!ok) set_err("format must be ZZ_ZLIB, ZZ_GZIP or ZZ_DEFLATE"); return ok; }
static bool dec_packet_ok(uint32_t P, uint32_t min) { const bool ok = P >= min && P <= ZZ_MAX_PACKET_SIZE; if (!ok) set_err("packet size must be " + std::to_string(min) + "..32768"); return ok; }
// zz_decode_device and zz_decode_points_device start here: the stats they report, the counter block, the trailer's verdict word
static int begin_decode_call(zz_ctx* c)
{
    auto& D = c->dec;
    D.last_path = 0; D.last_pending = 0; D.last_rounds = 0; D.last_index.clear();
    if (int rc = D.tot.grow(ZZ_TOT_SLOTS)) return rc;
    return D.ok.grow(1);
}
// The DEFLATE bytes a parallel path works on and where their packets start: an index of npk + 1 entries, or discovery's candidates
struct dec_stream { const uint8_t* s; uint64_t sn; const uint64_t* starts; uint64_t nstarts, npk; uint32_t P; };
// phase 1 and phase 2's workspace for `packets` packets (points: tiles) of `bytes` output bytes and `results` per-packet results. The
// range reads return a failure; the whole-stream and points paths go serial (dec_have).
static int dec_batch_workspace(zz_ctx* c, uint64_t packets, uint64_t bytes, uint32_t words, uint64_t results)
{
    auto& D = c->dec;
    if (int rc = D.st.grow(bytes)) return rc;
    if (int rc = D.pend.grow(packets * words)) return rc;
    if (int rc = D.pcnt.grow(packets)) return rc;
    if (int rc = D.prem.grow(packets)) return rc;
    if (int rc = D.ends.grow(results)) return rc;
    return D.stat.grow(results);
}
// phase 1's parameters but for the batch: the caller sets k0, npk, mode, dst, cap and ebase
static zz_inf_params dec_inf_params(zz_ctx* c, const dec_stream& S, uint32_t words)
{
    auto& D = c->dec;
    zz_inf_params Q = {};
    Q.s = S.s; Q.sn = S.sn; Q.starts = S.starts; Q.nstarts = S.nstarts; Q.npk_total = S.npk; Q.P = S.P;
    Q.st = D.st; Q.pend = D.pend; Q.words = words; Q.pcnt = D.pcnt; Q.prem = D.prem; Q.ends = D.ends; Q.stat = D.stat; Q.tot = D.tot;
    return Q;
}
// the counter block on the host: one copy, one wait
static int dec_read_tot(zz_ctx* c, unsigned long long (&tot)[ZZ_TOT_SLOTS], hipStream_t st)
{
    HIPCHK(hipMemcpyAsync(tot, c->dec.tot, sizeof tot, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}
// A checked read's sidecar (zz_inflate_check.h) and the container whose trailer it folds to, built by the checked entry points; the
// unchecked calls pass none (nullptr).
struct dec_sidecar { const uint32_t* cks; uint64_t L; int kind, format; };
// what the checked calls refuse before anything is launched, on top of the unchecked calls' own
static int dec_sidecar_args(const dec_sidecar& sc, uint64_t entries, uint32_t P)
{
    if (!sc.cks) { set_err("null argument"); return ZZ_E_ARG; }
    if (entries - 1 > 0x7fffffffull) { set_err("at most 2^31 - 1 packets"); return ZZ_E_ARG; }
    if (entries - 1 != zi_sidecar_entries(sc.L, P)) { set_err("the index's packets are not total_len's: entries - 1 != max(1, ceil(total_len / packet_size))"); return ZZ_E_ARG; }
    return ZZ_OK;
}
// The sidecar against the stream's trailer, enqueued: unpack, fold, verdict. The caller reads D.verdict[0] (1: it holds) with its
// next wait. A raw stream has no trailer: nothing is launched, and nothing is read.
static int dec_sidecar_fold(zz_ctx* c, const dec_sidecar& sc, uint64_t npk, uint32_t P, const uint8_t* trailer, hipStream_t st)
{
    auto& D = c->dec;
    if (sc.format == ZZ_DEFLATE) return ZZ_OK;
    if (int rc = D.side.grow(npk)) return rc;
    if (int rc = D.side_total.grow(1)) return rc;
    if (int rc = D.verdict.grow(2)) return rc;
    HIPCHK(hipMemsetAsync(D.verdict, 0, 8, st));
    hipLaunchKernelGGL(k_sidecar_unpack, dim3((uint32_t)((npk + 255) / 256)), dim3(256), 0, st, sc.cks, (uint32_t)npk, P, sc.L, sc.kind, D.side.p, D.verdict.p);
    hipLaunchKernelGGL(k_cks_reduce, dim3(1), dim3(ZZ_RED_THREADS), 0, st, D.side.p, (uint32_t)npk, P, sc.L, sc.kind, D.side_total.p);
    hipLaunchKernelGGL(k_sidecar_verdict, dim3(1), dim3(1), 0, st, trailer, sc.format, D.side_total.p, sc.L, D.verdict.p);
    HIPCHK(hipGetLastError());
    return ZZ_OK;
}
// The front of every indexed call: the index's two ends -- and the sidecar's verdict, its fold enqueued first -- read in one wait.
// What a mismatch means is the caller's: the serial path, an error, or every read's failure.
enum { DEC_FRONT_OK = 0, DEC_FRONT_ENDS = 1, DEC_FRONT_SIDECAR = 2 };       // (negative: a HIP error)
static int dec_index_front(zz_ctx* c, const dec_stream& S, const dec_sidecar* sc, hipStream_t st)
{
    uint64_t ends[2];
    uint32_t holds = 1;                                             // the sidecar folds to the trailer
    if (sc) if (int rc = dec_sidecar_fold(c, *sc, S.npk, S.P, S.s + S.sn, st)) return rc;
    HIPCHK(hipMemcpyAsync(&ends[0], S.starts, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&ends[1], S.starts + S.npk, 8, hipMemcpyDeviceToHost, st));
    if (sc && sc->format != ZZ_DEFLATE) HIPCHK(hipMemcpyAsync(&holds, c->dec.verdict.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ends[0] != 0 || ends[1] != S.sn) return DEC_FRONT_ENDS;
    return holds == 1 ? DEC_FRONT_OK : DEC_FRONT_SIDECAR;
}
static int dec_front_refused(int front)                             // (the range reads: either is ZZ_E_DATA)
{
    set_err(front == DEC_FRONT_ENDS ? "the index does not describe this stream: its ends are not the DEFLATE bytes' ends"
                                    : "the packet checksums do not describe this stream: they do not fold to its trailer (checksum or length)");
    return ZZ_E_DATA;
}

// phase 1 and phase 2 over S's packets [0, npk) (starts on the device). Indexed: per-packet results per batch,
// the last packet's kept in *last_stat; discovery: per candidate in dec.ends / dec.stat. Counters in dec.tot.
static int dec_packets(zz_ctx* c, const dec_stream& S, int mode, uint8_t* dst, uint64_t cap, hipStream_t st, uint32_t* rounds_launched,
                       uint32_t* last_stat)
{
    auto& D = c->dec;
    const uint32_t P = S.P;
    const zz_inf_geom geo = zz_inf_geometry(P, S.npk ? S.npk : 1);
    const uint64_t B = geo.B;
    const uint64_t per = mode == ZZ_INF_INDEXED ? B : S.npk;    // results kept per batch, or per candidate (bounded)
    if (!dec_have(dec_batch_workspace(c, B, B * P, geo.words, per))) return DEC_SERIAL;
    HIPCHK(hipMemsetAsync(D.tot, 0, ZZ_TOT_SLOTS * sizeof(unsigned long long), st));
    const uint32_t rounds = zz_inf_rounds(B);
    *rounds_launched = rounds;
    zz_inf_params Q = dec_inf_params(c, S, geo.words);
    Q.mode = mode; Q.dst = dst; Q.cap = cap;
    for (uint64_t k0 = 0; k0 < S.npk; k0 += B) {
        const uint32_t nb = (uint32_t)(S.npk - k0 < B ? S.npk - k0 : B);
        Q.k0 = k0; Q.npk = nb; Q.ebase = mode == ZZ_INF_INDEXED ? k0 : 0;
        hipLaunchKernelGGL(k_inflate_packets, dim3(nb), dim3(ZZ_INF_THREADS), geo.lds, st, Q);
        zz_res_params R{ dst, k0 * P, P, nb, geo.words, D.st, D.pend, D.pcnt, D.prem, D.tot };
        for (uint32_t r = 1; r <= rounds; ++r) hipLaunchKernelGGL(k_inflate_resolve, dim3(nb), dim3(ZZ_INF_RES_THREADS), 0, st, R, r);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(last_stat, D.stat + (S.npk - 1 - Q.ebase), 4, hipMemcpyDeviceToHost, st));
    return DEC_DONE;
}

// what dec_packets left for the packets [0, npk) it ran on (their chain already checked by the kernel or the host walk)
static int dec_collect(zz_ctx* c, uint64_t npk, uint32_t P, uint32_t rounds, uint32_t last, hipStream_t st, uint64_t* out)
{
    auto& D = c->dec;
    unsigned long long tot[ZZ_TOT_SLOTS];
    if (int rc = dec_read_tot(c, tot, st)) return rc;
    if (tot[ZZ_TOT_FAILED] != 0 || !(last & 1u) || !(last & 2u)) return DEC_SERIAL;
    *out = (npk - 1) * (uint64_t)P + (last >> 3);
    if (tot[ZZ_TOT_UNWRITTEN] != 0) return DEC_NOSPACE;
    if (tot[ZZ_TOT_OPEN + rounds] != 0) return DEC_SERIAL;  // (cannot happen: the rounds suffice for any chain)
    D.last_pending = tot[ZZ_TOT_PENDING];
    D.last_rounds = 0;
    if (tot[ZZ_TOT_PENDING]) { uint32_t r = 1; while (r < rounds && tot[ZZ_TOT_OPEN + r] != 0) ++r; D.last_rounds = r; }
    return DEC_DONE;
}

static int dec_indexed(zz_ctx* c, const uint8_t* s, uint64_t sn, const uint64_t* d_index, uint64_t entries, uint32_t P,
                       uint8_t* dst, uint64_t cap, hipStream_t st, uint64_t* out)
{
    if (entries < 2) return DEC_SERIAL;
    const uint64_t npk = entries - 1;
    if (npk > (1ull << 40)) return DEC_SERIAL;
    const dec_stream S{ s, sn, d_index, entries, npk, P };
    if (const int front = dec_index_front(c, S, nullptr, st)) return front < 0 ? front : DEC_SERIAL;
    uint32_t rounds = 0, last = 0;
    int rc = dec_packets(c, S, ZZ_INF_INDEXED, dst, cap, st, &rounds, &last);
    if (rc != DEC_DONE) return rc;
    return dec_collect(c, npk, P, rounds, last, st, out);
}

// discovery: candidates from the scan, phase 1 from every one of them (at its place if all are true starts), the chain
// of true starts walked on the host; if some candidates are not starts, phase 1 again on the index the walk recovered
static int dec_discover(zz_ctx* c, const uint8_t* s, uint64_t sn, uint32_t P, uint8_t* dst, uint64_t cap, hipStream_t st,
                        uint64_t* out)
{
    auto& D = c->dec;
    // a packet of P bytes takes at least P / 1032 + 6 bytes of stream (the longest match per two bits, the closing stored
    // block): twice the packets that can fit bounds the speculative work on adversarial input
    uint64_t cap_c = 2 * (sn / ((uint64_t)P / 1032 + 6)) + 64;
    if (cap_c > ZZ_INF_MAX_CANDIDATES) cap_c = ZZ_INF_MAX_CANDIDATES;
    if (!dec_have(D.cand.grow(cap_c + 1))) return DEC_SERIAL;
    HIPCHK(hipMemsetAsync(D.tot, 0, ZZ_TOT_SLOTS * sizeof(unsigned long long), st));
    {
        uint64_t g = (sn + 255) / 256;
        if (g > 8192) g = 8192;
        if (g == 0) g = 1;
        hipLaunchKernelGGL(k_inflate_scan, dim3((uint32_t)g), dim3(256), 0, st, s, sn, D.cand + 1, D.tot, cap_c);
    }
    HIPCHK(hipGetLastError());
    unsigned long long count = 0;
    HIPCHK(hipMemcpyAsync(&count, D.tot, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (count > cap_c) return DEC_SERIAL;
    std::vector<uint64_t> cand(count + 1);
    cand[0] = 0;                                             // the position behind the container header
    if (count) HIPCHK(hipMemcpyAsync(cand.data() + 1, D.cand + 1, count * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    const uint64_t nc = cand.size();
    HIPCHK(hipMemcpyAsync(D.cand, cand.data(), nc * 8, hipMemcpyHostToDevice, st));
    uint32_t rounds = 0, last = 0;
    int rc = dec_packets(c, dec_stream{ s, sn, D.cand, nc, nc, P }, ZZ_INF_DISCOVER, dst, cap, st, &rounds, &last);
    if (rc != DEC_DONE) return rc;
    std::vector<uint64_t> ends(nc);
    std::vector<uint32_t> stat(nc);
    HIPCHK(hipMemcpyAsync(ends.data(), D.ends, nc * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(stat.data(), D.stat, nc * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // walk from the first start: a true start ends exactly where the next true start begins. A candidate decoded at the
    // wrong place (behind false ones) may not have fit the destination; its end is known all the same.
    std::vector<uint64_t>& index = D.last_index;
    index.assign(1, 0);
    uint64_t i = 0;
    for (;;) {
        if (!(stat[i] & 1u)) return DEC_SERIAL;
        if (stat[i] & 2u) { if (ends[i] != sn) return DEC_SERIAL; break; }
        const auto it = std::lower_bound(cand.begin() + i + 1, cand.end(), ends[i]);
        if (it == cand.end() || *it != ends[i]) return DEC_SERIAL;
        i = (uint64_t)(it - cand.begin());
        index.push_back(cand[i]);
    }
    const uint64_t npk = index.size();
    index.push_back(sn);
    if (npk == nc) return dec_collect(c, npk, P, rounds, last, st, out);   // every candidate was a true start, decoded in place
    HIPCHK(hipMemcpyAsync(D.cand, index.data(), index.size() * 8, hipMemcpyHostToDevice, st));
    return dec_indexed(c, s, sn, D.cand, index.size(), P, dst, cap, st, out);
}

// The packet index the last zz_decode_device recovered by discovery (entries = packets + 1, as zz_packet_index_device)
extern "C" int zz_ctx_last_decode_index_device(zz_ctx* c, uint64_t* d_index, uint64_t max_entries, uint64_t* entries,
                                               void* hip_stream)
{
    if (!c || !entries) { set_err("null argument"); return ZZ_E_ARG; }
    if (c->dec.last_path != ZZ_DECODE_DISCOVERED) { set_err("the last decode on this context did not discover an index"); return ZZ_E_ARG; }
    const auto& v = c->dec.last_index;
    *entries = v.size();
    if (!d_index || max_entries < v.size()) { set_err("index buffer too small"); return ZZ_E_NOSPACE; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(hipMemcpyAsync(d_index, v.data(), v.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

// the decoded bytes against the trailer, on the device (zz_checksum.h's per-packet partials and their fold)
static int dec_check_trailer(zz_ctx* c, const uint8_t* trailer, int format, const uint8_t* dst, uint64_t n, hipStream_t st, bool* good)
{
    auto& D = c->dec;
    *good = true;
    if (format == ZZ_DEFLATE) return ZZ_OK;
    const int kind = cks_kind_for(format);
    const uint32_t CP = 32768;
    const uint64_t npk = (n + CP - 1) / CP;
    HIPCHK(hipMemsetAsync(c->d_cks_total, 0, sizeof(zz_cks_total), st));
    if (npk) {
        if (int rc = D.cks.grow(npk)) return rc;
        zz_packet_params pp = {};
        pp.src = dst; pp.n = n; pp.packet_size = CP; pp.npk = (uint32_t)npk; pp.cks_kind = kind; pp.cks = D.cks;
        launch_cks_partials(pp, 16384, st);
        launch_cks_fold(c, pp, kind, st);
    }
    hipLaunchKernelGGL(k_inflate_trailer, dim3(1), dim3(1), 0, st, trailer, format, c->d_cks_total, n, D.ok);
    HIPCHK(hipGetLastError());
    uint32_t ok = 0;
    HIPCHK(hipMemcpyAsync(&ok, D.ok, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *good = ok == 1;
    return ZZ_OK;
}

// the container header, read on the host (it may hold a file name of any length): *hl = its length; the stream holds at
// least the header and the trailer
static int dec_container(const uint8_t* d_src, uint64_t src_len, int format, hipStream_t st, int64_t* hl_out)
{
    int64_t hl = 0;
    if (format != ZZ_DEFLATE) {
        uint64_t have = src_len < 4096 ? src_len : 4096;
        std::vector<uint8_t> h;
        for (;;) {
            h.resize(have);
            if (have) HIPCHK(hipMemcpyAsync(h.data(), d_src, have, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            hl = zi_header(format, h.data(), have);
            if (hl != -1 || have == src_len) break;
            have = src_len - have < 3 * have ? src_len : 4 * have;
        }
        if (hl == -2) { set_err("the stream needs a preset dictionary (FDICT): not supported"); return ZZ_E_UNSUPPORTED; }
        if (hl < 0) { set_err("not a valid stream of the requested format: bad container header"); return ZZ_E_DATA; }
    }
    if (src_len < (uint64_t)hl + (uint64_t)trailer_len(format)) { set_err("not a valid stream of the requested format: truncated"); return ZZ_E_DATA; }
    *hl_out = hl;
    return ZZ_OK;
}

extern "C" int zz_decode_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, void* d_dst_v, uint64_t cap, uint64_t* out_len,
                                int format, uint32_t P, const uint64_t* d_index, uint64_t entries, void* hip_stream)
{
    if (!c || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    *out_len = 0;
    if (!dec_format_ok(format) || !dec_packet_ok(P, 0)) return ZZ_E_ARG;
    if ((!d_src_v && src_len) || (!d_dst_v && cap)) { set_err("null buffer"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    const uint8_t* d_src = (const uint8_t*)d_src_v;
    uint8_t* d_dst = (uint8_t*)d_dst_v;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& D = c->dec;
    if (int rc = begin_decode_call(c)) return rc;
    if (int rc = D.sres.grow(1)) return rc;
    int64_t hl = 0;
    if (int rc = dec_container(d_src, src_len, format, st, &hl)) return rc;
    const uint64_t tl = (uint64_t)trailer_len(format);
    const uint8_t* s = d_src + hl;
    const uint64_t sn = src_len - hl - tl;
    uint64_t out = 0;
    int got = DEC_SERIAL;
    if (P != 0 && sn > 0) {
        got = d_index ? dec_indexed(c, s, sn, d_index, entries, P, d_dst, cap, st, &out) : dec_discover(c, s, sn, P, d_dst, cap, st, &out);
        if (got < 0) return got;
        if (got == DEC_NOSPACE) {
            set_err("destination too small for the decoded stream (" + std::to_string(out) + " bytes)");
            return ZZ_E_NOSPACE;
        }
        if (got == DEC_DONE) D.last_path = d_index ? ZZ_DECODE_INDEXED : ZZ_DECODE_DISCOVERED;
    }
    if (got != DEC_DONE) {
        D.last_pending = 0; D.last_rounds = 0;
        hipLaunchKernelGGL(k_inflate_serial, dim3(1), dim3(ZZ_INF_THREADS), 0, st, s, src_len - hl, d_dst, cap, D.sres);
        HIPCHK(hipGetLastError());
        zz_inf_serial_out r;
        HIPCHK(hipMemcpyAsync(&r, D.sres, sizeof r, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (r.err == ZI_E_SPACE) { set_err("destination too small for the decoded stream"); return ZZ_E_NOSPACE; }
        if (r.err == ZI_E_FAR) { set_err("not a valid stream of the requested format: distance too far back"); return ZZ_E_DATA; }
        if (r.err) { set_err("not a valid stream of the requested format: invalid block structure"); return ZZ_E_DATA; }
        const uint64_t rest = src_len - hl >= r.end ? src_len - hl - r.end : 0;
        if (rest != tl) {
            set_err(rest < tl ? "not a valid stream of the requested format: truncated trailer"
                                                : "not a valid stream of the requested format: bytes behind the trailer");
            return ZZ_E_DATA;
        }
        out = r.out;
        D.last_path = ZZ_DECODE_SERIAL;
    }
    bool good = true;
    int rc = dec_check_trailer(c, d_src + src_len - tl, format, d_dst, out, st, &good);
    if (rc) return rc;
    if (!good) { set_err("not a valid stream of the requested format: checksum or ISIZE mismatch"); return ZZ_E_DATA; }
    *out_len = out;
    return ZZ_OK;
}

// ---- any stream through a point index (zz_inflate_points.h; the rules in zz_inflate_core.h) -----------------------------------
// The builder: one sequential pass on the host, no GPU, no context.
extern "C" int zz_points_index_host(const uint8_t* src, uint64_t src_len, int format, uint64_t spacing, uint64_t* points,
                                    uint64_t max_entries, uint64_t* entries, uint64_t* out_len)
{
    if (!entries || !out_len || (!src && src_len)) { set_err("null argument"); return ZZ_E_ARG; }
    *entries = 0; *out_len = 0;
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    if (spacing == 0) { set_err("spacing must be at least 1"); return ZZ_E_ARG; }
    struct sink_t { std::vector<uint64_t> rows; void put(uint64_t bit, uint64_t pos) { rows.push_back(bit); rows.push_back(pos); } } sink;
    std::vector<uint8_t> ring(ZI_RING);
    std::vector<zi_tables> S(1);
    std::vector<zi_sum> sum(1);
    uint64_t n = 0;
    const int rc = zi_points_build(src, src_len, format, spacing, sink, ring.data(), S[0], sum[0], &n);
    if (rc == ZI_ITEM_UNSUPPORTED) { set_err("the stream needs a preset dictionary (FDICT): not supported"); return ZZ_E_UNSUPPORTED; }
    if (rc) { set_err("not a valid stream of the requested format"); return ZZ_E_DATA; }
    *entries = sink.rows.size() / 2;
    *out_len = n;
    if (!points || max_entries < *entries) { set_err("point index buffer too small"); return ZZ_E_NOSPACE; }
    memcpy(points, sink.rows.data(), sink.rows.size() * 8);
    return ZZ_OK;
}

// One batch of the point-index decode, shared by dec_points and the sidecar's builder (pw_build): segments [0, nseg) of `rows` (host,
// nseg + 1 of them) through phase 1, the tile counts and the rounds onto dst, which is addressed by absolute output position. The
// workspace (dec_points_workspace) holds the batch. DEC_SERIAL: a segment's run was refused. *pending, *rounds_used: what the batch adds.
static int dec_points_workspace(zz_ctx* c, uint64_t max_bytes, uint64_t max_segs)
{
    auto& D = c->dec;
    const uint64_t max_tiles = (max_bytes + ZI_POINTS_TILE - 1) / ZI_POINTS_TILE;
    if (int rc = dec_batch_workspace(c, max_tiles, max_bytes, ZI_POINTS_TILE / 32, 0)) return rc;
    if (int rc = D.pts.rows.grow(2 * (max_segs + 1))) return rc;
    if (int rc = D.pts.stat.grow(max_segs)) return rc;
    return D.pts.next.grow(1);
}
static int dec_points_batch(zz_ctx* c, const uint8_t* s, uint64_t sn, const uint64_t* rows, uint32_t nseg, bool last, uint8_t* dst,
                            hipStream_t st, uint64_t* pending, uint32_t* rounds_used)
{
    auto& D = c->dec;
    const uint32_t words = ZI_POINTS_TILE / 32;
    const uint64_t resident = 256ull * ZZ_PT_WG_PER_CU;                     // persistent wavefronts: what the CUs hold at once
    const uint64_t base = rows[1], nbytes = rows[2 * (uint64_t)nseg + 1] - base;
    const uint32_t tiles = (uint32_t)((nbytes + ZI_POINTS_TILE - 1) / ZI_POINTS_TILE);
    HIPCHK(hipMemsetAsync(D.tot, 0, ZZ_TOT_SLOTS * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(D.pts.next, 0, sizeof(unsigned int), st));
    if (tiles) HIPCHK(hipMemsetAsync(D.pend, 0, (uint64_t)tiles * words * 4, st));
    HIPCHK(hipMemcpyAsync(D.pts.rows, rows, (uint64_t)(nseg + 1) * 16, hipMemcpyHostToDevice, st));
    zz_pt_params Q;
    Q.s = s; Q.sn = sn; Q.rows = D.pts.rows; Q.nseg = nseg; Q.last = last; Q.dst = dst; Q.base = base; Q.nbytes = nbytes;
    Q.st = D.st; Q.pend = D.pend; Q.words = (uint64_t)tiles * words; Q.stat = D.pts.stat; Q.next = D.pts.next; Q.tot = D.tot;
    hipLaunchKernelGGL(k_inflate_segments, dim3((uint32_t)(nseg < resident ? nseg : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
    if (tiles) hipLaunchKernelGGL(k_points_count, dim3(tiles), dim3(256), 0, st, D.pend, D.pcnt, D.prem, D.tot);
    HIPCHK(hipGetLastError());
    unsigned long long tot[ZZ_TOT_SLOTS];
    if (int rc = dec_read_tot(c, tot, st)) return rc;
    if (tot[ZZ_TOT_FAILED] != 0) return DEC_SERIAL;                         // a segment is not what the index says
    if (tot[ZZ_TOT_PENDING] == 0) return DEC_DONE;
    const uint32_t rounds = zz_inf_rounds(nseg);                            // a chain has at most one link per segment of a batch
    zz_res_params R{ dst, base, ZI_POINTS_TILE, tiles, words, D.st, D.pend, D.pcnt, D.prem, D.tot };
    for (uint32_t r = 1; r <= rounds; ++r) hipLaunchKernelGGL(k_inflate_resolve, dim3(tiles), dim3(ZZ_INF_RES_THREADS), 0, st, R, r);
    HIPCHK(hipGetLastError());
    if (int rc = dec_read_tot(c, tot, st)) return rc;
    if (tot[ZZ_TOT_OPEN + rounds] != 0) return DEC_SERIAL;                  // (cannot happen: the rounds suffice for any chain)
    uint32_t r = 1;
    while (r < rounds && tot[ZZ_TOT_OPEN + r] != 0) ++r;
    *pending += tot[ZZ_TOT_PENDING];
    *rounds_used = std::max(*rounds_used, r);
    return DEC_DONE;
}

// phase 1 over the segments, the tile counts and the rounds, batch by batch. DEC_SERIAL: the index or a segment's run was refused
// (what this wrote so far lies inside [0, cap) and the serial path writes over it).
static int dec_points(zz_ctx* c, const uint8_t* s, uint64_t sn, const uint64_t* points, uint64_t entries, uint8_t* dst, uint64_t cap,
                      hipStream_t st, uint64_t* out)
{
    auto& D = c->dec;
    if (!zi_points_check(points, entries, sn, cap, ZZ_INF_BATCH_BYTES)) return DEC_SERIAL;
    const uint64_t nseg_total = entries - 1;
    if ((points[2 * nseg_total] + 7) / 8 != sn) return DEC_SERIAL;          // the trailer begins behind the final block's last byte
    uint64_t max_bytes = 1, max_segs = 1;
    for (uint64_t k0 = 0, k1; k0 < nseg_total; k0 = k1) {
        k1 = zi_points_batches(points, entries, k0, ZZ_INF_BATCH_BYTES, ZZ_PT_BATCH_SEGMENTS);
        max_bytes = std::max(max_bytes, points[2 * k1 + 1] - points[2 * k0 + 1]);
        max_segs = std::max(max_segs, k1 - k0);
    }
    if (!dec_have(dec_points_workspace(c, max_bytes, max_segs))) return DEC_SERIAL;
    uint64_t pending = 0;
    uint32_t rounds_used = 0;
    for (uint64_t k0 = 0, k1; k0 < nseg_total; k0 = k1) {
        k1 = zi_points_batches(points, entries, k0, ZZ_INF_BATCH_BYTES, ZZ_PT_BATCH_SEGMENTS);
        const int got = dec_points_batch(c, s, sn, points + 2 * k0, (uint32_t)(k1 - k0), k1 == nseg_total, dst, st, &pending, &rounds_used);
        if (got != DEC_DONE) return got;
    }
    D.last_pending = pending; D.last_rounds = rounds_used;
    *out = points[2 * nseg_total + 1];
    return DEC_DONE;
}

extern "C" int zz_decode_points_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, void* d_dst_v, uint64_t cap, uint64_t* out_len,
                                       int format, const uint64_t* points, uint64_t entries, void* hip_stream)
{
    if (!c || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    *out_len = 0;
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    if (!d_src_v || (!d_dst_v && cap)) { set_err("null buffer"); return ZZ_E_ARG; }
    if (!points || entries < 2) { set_err("a point index has at least two rows (host memory)"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    const uint8_t* d_src = (const uint8_t*)d_src_v;
    uint8_t* d_dst = (uint8_t*)d_dst_v;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& D = c->dec;
    if (int rc = begin_decode_call(c)) return rc;
    int64_t hl = 0;
    if (int rc = dec_container(d_src, src_len, format, st, &hl)) return rc;
    const uint64_t tl = (uint64_t)trailer_len(format);
    const uint64_t sn = src_len - hl - tl;
    uint64_t out = 0;
    int got = dec_points(c, d_src + hl, sn, points, entries, d_dst, cap, st, &out);
    if (got < 0) return got;
    if (got == DEC_DONE) {
        bool good = true;
        if (int rc = dec_check_trailer(c, d_src + src_len - tl, format, d_dst, out, st, &good)) return rc;
        if (good) { D.last_path = ZZ_DECODE_POINTS; *out_len = out; return ZZ_OK; }
    }
    // the index, a segment or the checksum was refused: the serial path decides the result, as if no index had been given
    return zz_decode_device(c, d_src_v, src_len, d_dst_v, cap, out_len, format, 0, nullptr, 0, hip_stream);
}

// ---- the point index built on the device (zz_inflate_points_find.h; the rules in zz_inflate_core.h) -----------------------------
extern "C" uint64_t zz_points_index_bound(uint64_t src_len, uint64_t chunk_bytes)
{
    return chunk_bytes < 16 ? 0 : zi_find_chunks(src_len, chunk_bytes) + 1;
}

// one round's jobs: up, one launch, the results back in place (want[0, n))
static int pf_run_jobs(zz_ctx* c, const uint8_t* d, uint64_t n, zi_find_job* want, uint64_t njobs, hipStream_t st)
{
    auto& F = c->dec.pf;
    HIPCHK(hipMemcpyAsync(F.job, want, njobs * sizeof(zi_find_job), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(F.next, 0, sizeof(unsigned int), st));
    zz_pf_params Q = {};
    Q.d = d; Q.n = n; Q.job = F.job; Q.njobs = (uint32_t)njobs; Q.next = F.next;
    const uint64_t resident = 256ull * ZZ_PF_WG_PER_CU;
    hipLaunchKernelGGL(k_points_reach, dim3((uint32_t)(njobs < resident ? njobs : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(want, F.job, njobs * sizeof(zi_find_job), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

extern "C" int zz_points_index_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint64_t chunk_bytes, uint64_t spacing,
                                      uint64_t* points, uint64_t max_entries, uint64_t* entries, uint64_t* out_len, void* hip_stream)
{
    if (!c || !d_src_v || !entries || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    *entries = 0; *out_len = 0;
    if (chunk_bytes < 16) { set_err("chunk_bytes must be at least 16"); return ZZ_E_ARG; }
    if (spacing == 0) { set_err("spacing must be at least 1"); return ZZ_E_ARG; }
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    if (call_pending(c)) return ZZ_E_ARG;
    const uint8_t* d_src = (const uint8_t*)d_src_v;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& F = c->dec.pf;
    F.candidates = 0; F.dropped = 0; F.rounds = 0;
    int64_t hl = 0;
    if (int rc = dec_container(d_src, src_len, format, st, &hl)) return rc;
    const uint8_t* d = d_src + hl;                                          // D: the DEFLATE bytes and the trailer
    const uint64_t n = src_len - (uint64_t)hl;
    const uint64_t chunks = zi_find_chunks(n, chunk_bytes);
    if (n > (~0ull >> 3) || chunks > 0x7fffffffull) { set_err("at most 2^31 - 1 chunks"); return ZZ_E_ARG; }
    if (int rc = F.job.grow(chunks + 2)) return rc;
    if (int rc = F.next.grow(1)) return rc;
    const uint64_t resident = 256ull * ZZ_PF_WG_PER_CU;
    // the candidates
    std::vector<zi_find_job> rec(chunks + 2);
    std::vector<uint64_t> cand{ 0 };
    if (chunks > 1) {
        HIPCHK(hipMemsetAsync(F.next, 0, sizeof(unsigned int), st));
        zz_pf_params Q = {};
        Q.d = d; Q.n = n; Q.chunk = chunk_bytes; Q.chunks = chunks; Q.job = F.job; Q.next = F.next;
        hipLaunchKernelGGL(k_points_find, dim3((uint32_t)(chunks - 1 < resident ? chunks - 1 : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rec.data(), F.job, chunks * sizeof(zi_find_job), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint64_t k = 1; k < chunks; ++k) if (rec[k].a != ZI_FIND_NONE) cand.push_back(rec[k].a);
    }
    // the jobs, the chain and its repair rounds
    const uint64_t nc = cand.size();
    std::vector<zi_find_job> rc_(nc), rr_(nc + 1);
    std::vector<uint64_t> acc(2 * (2 * nc + 2));
    memset(rc_.data(), 0, nc * sizeof(zi_find_job)); memset(rr_.data(), 0, (nc + 1) * sizeof(zi_find_job));
    zi_find_walk W{ zi_view<const uint64_t>{ cand.data(), nc }, nc, zi_view<zi_find_job>{ rc_.data(), nc }, zi_view<zi_find_job>{ rr_.data(), nc + 1 },
                    zi_view<uint64_t>{ acc.data(), acc.size() }, 0, 0, 0, 0, 0, 0, chunk_bytes };
    uint64_t nwant = nc;
    for (uint64_t k = 0; k < nc; ++k) rec[k] = zi_find_first_job(W.cand, nc, k, W.slack, n);
    int verdict;
    for (;;) {
        ++F.rounds;
        if (int rc = pf_run_jobs(c, d, n, rec.data(), nwant, st)) return rc;
        for (uint64_t j = 0; j < nwant; ++j) zi_find_store(W, rec[j]);
        verdict = zi_find_link(W, zi_view<zi_find_job>{ rec.data(), rec.size() }, &nwant);
        if (verdict != ZI_FW_MORE) break;
        if (F.rounds > 3 * nc + 2) { set_err("the chain of block starts did not close"); return ZZ_E_DATA; }   // (every round confirms a job)
    }
    F.candidates = nc; F.dropped = nc - W.kept;
    if (verdict == ZI_FW_DATA) { set_err("not a valid stream of the requested format"); return ZZ_E_DATA; }
    uint8_t t[8] = { 0 };
    const uint64_t tn = n < 8 ? n : 8;
    if (tn) HIPCHK(hipMemcpyAsync(t + 8 - tn, d + n - tn, tn, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!zi_find_trailer_ok(format, n, W.end_bit, W.bytes, t)) { set_err("not a valid stream of the requested format: trailer"); return ZZ_E_DATA; }
    *entries = zi_find_rows(W, spacing, nullptr, 0);
    *out_len = W.bytes;
    if (!points || max_entries < *entries) { set_err("point index buffer too small"); return ZZ_E_NOSPACE; }
    zi_find_rows(W, spacing, points, max_entries);
    return ZZ_OK;
}

extern "C" int zz_ctx_last_points_index_stats(const zz_ctx* c, uint64_t* candidates, uint64_t* dropped, uint32_t* rounds)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (candidates) *candidates = c->dec.pf.candidates;
    if (dropped) *dropped = c->dec.pf.dropped;
    if (rounds) *rounds = c->dec.pf.rounds;
    return ZZ_OK;
}

// ---- bytes [first, first + nbytes) of an indexed stream (zz_inflate.h's range kernels; the rules in zz_inflate_core.h) -----
// One attempt: packets [kb, k1) through phase 1 and the rounds, batch by batch, onto the stage; the window's bytes of every batch
// but the last go to d_dst at once (such a batch holds full packets only), the last batch's after the host has seen the
// attempt's counters: *ext = external bytes inside the window (then nothing more is copied: the caller tries again),
// *m = the bytes the range holds.
// Stage packets [0, n) at `stage` (phase 1's words at `stat`) summed into D.scks: the MAP forms of zz_checksum.h's bodies.
static void dec_stage_sums(zz_ctx* c, const dec_sidecar& sc, const uint8_t* stage, const uint32_t* stat, const zi_read_desc* desc, uint32_t n,
                           uint32_t P, hipStream_t st)
{
    zz_packet_params pp = {};
    pp.src = stage; pp.packet_size = P; pp.npk = n; pp.cks_kind = sc.kind; pp.cks = c->dec.scks;
    zz_stage_map M{ stat, desc, n };
    if (sc.kind == ZZ_CKS_CRC) hipLaunchKernelGGL(k_crc32_stage, dim3(n < 2048 ? n : 2048), dim3(ZZ_CRC_THREADS), 0, st, pp, M);
    else hipLaunchKernelGGL(k_adler_stage, dim3(n < 16384 ? n : 16384), dim3(ZZ_WAVE), 0, st, pp, M);
}

static int dec_range_attempt(zz_ctx* c, const dec_stream& S, uint64_t kb, uint64_t k1, uint64_t first, uint64_t nbytes, uint8_t* dst,
                             uint64_t cap, hipStream_t st, const dec_sidecar* sc, uint64_t* ext, uint64_t* pending, uint64_t* m, uint64_t* bad)
{
    auto& D = c->dec;
    const uint32_t P = S.P;
    const uint64_t npk = S.npk;
    const zz_inf_geom geo = zz_inf_geometry(P, k1 - kb);
    const uint64_t B = geo.B;
    if (int rc = D.stage.grow(ZI_BIAS + B * P + 16)) return rc;
    if (int rc = dec_batch_workspace(c, B, B * P, geo.words, B)) return rc;
    if (sc) if (int rc = D.scks.grow(B)) return rc;
    HIPCHK(hipMemsetAsync(D.tot, 0, ZZ_TOT_SLOTS * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(D.xcarry, 0xFF, ZI_BIAS / 8, st));   // the first batch: whatever lies below it is external
    const uint32_t rounds = zz_inf_rounds(B);
    const uint64_t k0 = first / P;
    const uint64_t wend = nbytes < k1 * P - first ? first + nbytes : k1 * P;       // the window's end, as far as packets go
    uint64_t xlo = 0, xhi = 0;                                  // where an external byte sends the call back: the window, or its packets whole
    zi_checked_window(sc != nullptr, first, nbytes, P, k0, k1, &xlo, &xhi);
    zz_inf_params Q = dec_inf_params(c, S, geo.words);
    Q.mode = ZZ_INF_INDEXED; Q.dst = D.stage + ZI_BIAS;
    for (uint64_t kf = kb; kf < k1; kf += B) {
        const uint32_t nb = (uint32_t)(k1 - kf < B ? k1 - kf : B);
        const uint64_t base = kf * P;
        Q.k0 = kf; Q.npk = nb; Q.cap = (uint64_t)nb * P; Q.ebase = kf;
        hipLaunchKernelGGL(k_inflate_packets_range, dim3(nb), dim3(ZZ_INF_THREADS), geo.lds, st, Q);
        zz_res_params R{ D.stage, ZI_BIAS, P, nb, geo.words, D.st, D.pend, D.pcnt, D.prem, D.tot };
        zz_res_range X{ D.xcarry, (int64_t)xlo - (int64_t)base, (int64_t)xhi - (int64_t)base };
        for (uint32_t r = 1; r <= rounds; ++r) hipLaunchKernelGGL(k_inflate_resolve_range, dim3(nb), dim3(ZZ_INF_RES_THREADS), 0, st, R, X, r);
        if (sc && kf + nb > k0) {                                   // the batch's touched packets: summed, held to the sidecar (ZZ_TOT_BAD_SUM)
            const uint32_t skip = (uint32_t)(k0 > kf ? k0 - kf : 0), n = nb - skip;
            dec_stage_sums(c, *sc, D.stage + ZI_BIAS + (uint64_t)skip * P, D.stat + skip, nullptr, n, P, st);
            zz_chk_params C{ sc->cks, npk, sc->L, P, sc->kind, D.scks.p, D.stat + skip };
            hipLaunchKernelGGL(k_stage_check_range, dim3((n + 255) / 256), dim3(256), 0, st, C, kf + skip, n, D.tot + ZZ_TOT_BAD_SUM);
        }
        // this batch's share of the window: stream bytes [lo, hi)
        const uint64_t lo = first > base ? first : base;
        uint64_t hi = base + (uint64_t)nb * P < wend ? base + (uint64_t)nb * P : wend;
        const bool last = kf + nb == k1;
        if (last) {
            unsigned long long tot[ZZ_TOT_SLOTS];
            uint32_t stat = 0;
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(tot, D.tot, sizeof tot, hipMemcpyDeviceToHost, st));     // (not dec_read_tot: the last packet's word rides behind it)
            HIPCHK(hipMemcpyAsync(&stat, D.stat + (nb - 1), 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (tot[ZZ_TOT_FAILED] != 0) { set_err("not a valid stream of the requested format: " + std::to_string(tot[ZZ_TOT_FAILED]) + " of the range's packets do not decode as the index says"); return ZZ_E_DATA; }
            if (tot[ZZ_TOT_OPEN + rounds] != 0) { set_err("pending bytes left unresolved"); return ZZ_E_DATA; }   // (cannot happen: the rounds suffice for any chain)
            *ext = tot[ZZ_TOT_EXTERNAL]; *pending = tot[ZZ_TOT_PENDING]; *bad = tot[ZZ_TOT_BAD_SUM];
            uint64_t have = nbytes;                                 // bytes of the stream from `first` on, if its end is in sight
            if (k1 == npk) { const uint64_t L = (npk - 1) * (uint64_t)P + (stat >> 3); have = L > first ? L - first : 0; }
            *m = nbytes < have ? nbytes : have;
            if (*ext != 0 || *bad != 0) return ZZ_OK;             // nothing more is copied: the caller tries again, or refuses
            if (hi > first + *m) hi = first + *m;
        }
        if (hi > first && hi - first > cap) hi = first + cap;                     // nothing past cap, whatever the call's result will be
        if (hi > lo) {
            const uint64_t n = hi - lo;
            uint64_t g = (n / 16 + 255) / 256;
            if (g > 4096) g = 4096;
            if (g == 0) g = 1;
            hipLaunchKernelGGL(k_inflate_range_copy, dim3((uint32_t)g), dim3(256), 0, st, D.stage + ZI_BIAS + (lo - base), dst + (lo - first), n);
        }
        if (!last) hipLaunchKernelGGL(k_inflate_range_carry, dim3(ZI_BIAS / 256), dim3(256), 0, st, D.stage.p, (uint64_t)nb * P, P, geo.words,
                                      D.st.p, D.pend.p, D.pcnt.p, D.xcarry.p);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

// zz_decode_range_device (sc == nullptr) and zz_decode_range_checked_device: one body
static int dec_range(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint32_t P,
                     const uint64_t* d_index, uint64_t entries, const dec_sidecar* sc,
                     uint64_t first, uint64_t nbytes, void* d_dst_v, uint64_t cap, uint64_t* out_len, void* hip_stream)
{
    if (!c || !d_src_v || !d_index || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    *out_len = 0;
    if (!dec_packet_ok(P, 1) || !dec_format_ok(format)) return ZZ_E_ARG;
    if (entries < 2) { set_err("the index needs at least two entries (packets + 1)"); return ZZ_E_ARG; }
    const uint64_t npk = entries - 1;
    if (first / P >= npk) { set_err("the range starts behind the index's last packet"); return ZZ_E_ARG; }
    if (first + nbytes < first) { set_err("first + nbytes overflows"); return ZZ_E_ARG; }
    if (!d_dst_v && cap) { set_err("null buffer"); return ZZ_E_ARG; }
    if (sc) if (int rc = dec_sidecar_args(*sc, entries, P)) return rc;
    if (nbytes == 0) return ZZ_OK;                                  // nothing to do: the context is not looked at
    if (call_pending(c)) return ZZ_E_ARG;
    const uint8_t* d_src = (const uint8_t*)d_src_v;
    uint8_t* d_dst = (uint8_t*)d_dst_v;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& D = c->dec;
    if (int rc = D.tot.grow(ZZ_TOT_SLOTS)) return rc;
    if (int rc = D.xcarry.grow(ZI_BIAS / 32)) return rc;
    int64_t hl = 0;
    if (int rc = dec_container(d_src, src_len, format, st, &hl)) return rc;
    const dec_stream S{ d_src + hl, src_len - hl - (uint64_t)trailer_len(format), d_index, entries, npk, P };
    const int front = dec_index_front(c, S, sc, st);
    if (front < 0) return front;
    if (front == DEC_FRONT_SIDECAR) *out_len = ~0ull;
    if (front) return dec_front_refused(front);
    const uint64_t k0 = first / P;
    const uint64_t lastk = (first + nbytes - 1) / P;
    const uint64_t k1 = lastk + 1 < npk ? lastk + 1 : npk;
    uint64_t h = zi_range_first_lookback(P, k0);
    for (uint32_t tries = 1;; ++tries) {
        const uint64_t kb = k0 - h;
        uint64_t ext = 0, pending = 0, m = 0, bad = 0;
        if (int rc = dec_range_attempt(c, S, kb, k1, first, nbytes, d_dst, cap, st, sc, &ext, &pending, &m, &bad)) {
            if (sc && rc == ZZ_E_DATA) *out_len = ~0ull;
            return rc;
        }
        if (ext != 0) {
            if (kb == 0) { set_err("not a valid stream of the requested format: a reference in front of the stream"); return ZZ_E_DATA; }   // (phase 1 refuses these)
            h = zi_range_next_lookback(h, k0);
            continue;
        }
        if (bad != 0) {
            *out_len = ~0ull;
            set_err("checksum mismatch: " + std::to_string(bad) + " of the range's packets do not decode to the bytes their checksums (or total_len) describe");
            return ZZ_E_DATA;
        }
        if (m > cap) {
            *out_len = ~0ull;
            set_err("destination too small for the range (" + std::to_string(m) + " bytes)");
            return ZZ_E_NOSPACE;
        }
        D.range.first_packet = kb; D.range.packets = k1 - kb; D.range.attempts = tries; D.range.pending = pending;
        *out_len = m;
        return ZZ_OK;
    }
}

extern "C" int zz_decode_range_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint32_t P,
                                      const uint64_t* d_index, uint64_t entries, uint64_t first, uint64_t nbytes,
                                      void* d_dst_v, uint64_t cap, uint64_t* out_len, void* hip_stream)
{
    return dec_range(c, d_src_v, src_len, format, P, d_index, entries, nullptr, first, nbytes, d_dst_v, cap, out_len, hip_stream);
}
extern "C" int zz_decode_range_checked_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint32_t P,
                                              const uint64_t* d_index, uint64_t entries, const uint32_t* d_cks, uint64_t total_len,
                                              uint64_t first, uint64_t nbytes, void* d_dst_v, uint64_t cap, uint64_t* out_len, void* hip_stream)
{
    const dec_sidecar sc{ d_cks, total_len, zi_sidecar_kind(format), format };
    return dec_range(c, d_src_v, src_len, format, P, d_index, entries, &sc, first, nbytes, d_dst_v, cap, out_len, hip_stream);
}

extern "C" int zz_ctx_last_decode_range_stats(const zz_ctx* c, uint64_t* first_packet, uint64_t* packets, uint32_t* attempts,
                                              uint64_t* pending_bytes)
{
    if (!c) { set_err("null context"); return ZZ_E_ARG; }
    if (first_packet) *first_packet = c->dec.range.first_packet;
    if (packets) *packets = c->dec.range.packets;
    if (attempts) *attempts = c->dec.range.attempts;
    if (pending_bytes) *pending_bytes = c->dec.range.pending;
    return ZZ_OK;
}

// ---- many reads of one indexed stream in one call (zz_inflate_ranges.h; the rules in zz_inflate_core.h) -------------------
// A read's own failure is worded "reads: ..." in zz_last_error (the Python layer tells it from a failure of the call by that).
// Per attempt: the plan, one wait for its totals and wave table, then per wave descriptors, phase 1, the rounds, the verdict and
// the copy, nothing of which the host waits for; the next attempt's plan finds what is left.
// zz_decode_ranges_device (sc == nullptr) and zz_decode_ranges_checked_device: one body
static_assert(ZI_CKS_ADLER == ZZ_CKS_ADLER && ZI_CKS_CRC == ZZ_CKS_CRC, "the sidecar's kinds are the checksum kernels'");
static int dec_ranges(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint32_t P,
                      const uint64_t* d_index, uint64_t entries, const dec_sidecar* sc,
                      uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                      void* const* d_dsts, const uint64_t* d_caps,
                      uint64_t* d_out_lens, int32_t* d_status, void* hip_stream)
{
    if (!c || !d_src_v || !d_index || !d_firsts || !d_nbytes || !d_dsts || !d_caps || !d_out_lens) { set_err("null argument"); return ZZ_E_ARG; }
    if (!dec_packet_ok(P, 1) || !dec_format_ok(format)) return ZZ_E_ARG;
    if (entries < 2) { set_err("the index needs at least two entries (packets + 1)"); return ZZ_E_ARG; }
    if (nranges > 0x7fffffffull) { set_err("at most 2^31 - 1 reads per call"); return ZZ_E_ARG; }
    if (sc) if (int rc = dec_sidecar_args(*sc, entries, P)) return rc;
    if (nranges == 0) return ZZ_OK;                                 // nothing to do: the context is not looked at
    if (call_pending(c)) return ZZ_E_ARG;
    const uint64_t npk = entries - 1;
    const uint8_t* d_src = (const uint8_t*)d_src_v;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& D = c->dec;
    D.ranges.packets = 0; D.ranges.retried = 0; D.ranges.attempts = 0; D.ranges.waves = 0;
    // a failure of the call itself: every read gets the code
    auto fail_all = [&](int code) -> int {
        hipLaunchKernelGGL(k_ranges_fill, dim3((uint32_t)std::min<uint64_t>((nranges + 255) / 256, 4096)), dim3(256), 0, st, d_out_lens, d_status,
                           nranges, (int32_t)code);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return code;
    };
    int64_t hl = 0;
    if (int rc = dec_container(d_src, src_len, format, st, &hl)) {
        if (rc == ZZ_E_DATA || rc == ZZ_E_UNSUPPORTED) return fail_all(rc);
        return rc;
    }
    const dec_stream S{ d_src + hl, src_len - hl - (uint64_t)trailer_len(format), d_index, entries, npk, P };
    const int front = dec_index_front(c, S, sc, st);
    if (front < 0) return front;
    if (front) return fail_all(dec_front_refused(front));
    if (int rc = D.tot.grow(ZZ_TOT_SLOTS)) return rc;
    if (int rc = D.rng_reads.grow(nranges)) return rc;
    if (int rc = D.rng_tot.grow(1)) return rc;
    if (int rc = D.rng_host.grow(1)) return rc;
    const zz_inf_geom geo = zz_inf_geometry(P, ~0ull);
    zz_rng_params Q{ d_firsts, d_nbytes, (uint8_t* const*)d_dsts, d_caps, d_out_lens, d_status, nranges, npk, P, geo.B, geo.B, D.rng_reads, D.rng_tot,
                     sc ? sc->cks : nullptr, sc ? sc->L : 0 };
    const zz_rng_totals& T = *D.rng_host.p;
    for (uint32_t tries = 1;; ++tries) {
        hipLaunchKernelGGL(k_ranges_plan, dim3(1), dim3(ZZ_RNG_PLAN_THREADS), 0, st, Q, tries == 1 ? 1 : 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(D.rng_host.p, D.rng_tot.p, sizeof(zz_rng_totals), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (T.nwaves == 0) {
            if (T.deferred != 0) { set_err("range plan made no progress"); return ZZ_E_HIP; }    // (cannot happen: wave 0 always takes a segment)
            break;
        }
        D.ranges.attempts = tries; D.ranges.packets += T.stage_end;
        const uint32_t rounds = zz_inf_rounds(T.longest);
        // the workspace follows the attempt's largest wave (nothing is grown while a wave's kernels run)
        uint64_t big = 0, prev = T.stage_end;
        for (uint64_t w = T.nwaves; w-- > 0;) {
            if (T.wave_first[w] == ~0ull) continue;
            big = std::max<uint64_t>(big, prev - T.wave_first[w]);
            prev = T.wave_first[w];
        }
        if (int rc = D.stage.grow(big * P + 16)) return rc;
        if (int rc = dec_batch_workspace(c, big, big * P, geo.words, big)) return rc;
        if (int rc = D.rng_desc.grow(big)) return rc;
        if (sc) if (int rc = D.scks.grow(big)) return rc;
        zz_inf_params I = dec_inf_params(c, S, geo.words);      // (k0 = 0, ebase = 0: a wave's packets are its descriptors')
        I.mode = ZZ_INF_INDEXED; I.dst = D.stage;
        for (uint64_t w = 0; w < T.nwaves; ++w) {
            if (T.wave_first[w] == ~0ull) continue;                 // (a segment longer than a wave's capacity went over it)
            uint64_t nx = w + 1;
            while (nx < T.nwaves && T.wave_first[nx] == ~0ull) ++nx;
            const uint64_t g0 = T.wave_first[w], g1 = nx < T.nwaves ? T.wave_first[nx] : T.stage_end;
            const uint64_t rlo = T.wave_read[w], rhi = nx < T.nwaves ? T.wave_read[nx] : nranges;
            const uint32_t nb = (uint32_t)(g1 - g0);                // < 2 * B, <= big
            ++D.ranges.waves;
            hipLaunchKernelGGL(k_ranges_desc, dim3((nb + 255) / 256), dim3(256), 0, st, Q, g0, nb, rlo, rhi, D.rng_desc.p);
            I.npk = nb; I.cap = (uint64_t)nb * P;
            zz_inf_ranges X{ D.rng_desc.p, D.rng_reads.p };
            hipLaunchKernelGGL(k_inflate_packets_ranges, dim3(nb), dim3(ZZ_INF_THREADS), geo.lds, st, I, X);
            zz_res_params R{ D.stage, 0, P, nb, geo.words, D.st, D.pend, D.pcnt, D.prem, D.tot };
            for (uint32_t r = 1; r <= rounds; ++r) hipLaunchKernelGGL(k_inflate_resolve_ranges, dim3(nb), dim3(ZZ_INF_RES_THREADS), 0, st, R, X, r);
            if (sc) {                                               // the wave's touched packets: summed, a mismatch charged to the read
                dec_stage_sums(c, *sc, D.stage, D.stat, D.rng_desc.p, nb, P, st);
                zz_chk_params C{ sc->cks, npk, sc->L, P, sc->kind, D.scks.p, D.stat.p };
                hipLaunchKernelGGL(k_stage_check_ranges, dim3((nb + 255) / 256), dim3(256), 0, st, C, D.rng_desc.p, nb, D.rng_reads.p);
            }
            hipLaunchKernelGGL(k_ranges_verdict, dim3((uint32_t)((rhi - rlo + 255) / 256)), dim3(256), 0, st, Q, g0, rlo, rhi, D.stat.p);
            hipLaunchKernelGGL(k_ranges_copy, dim3(nb), dim3(256), 0, st, Q, D.rng_desc.p, D.stage.p);
            HIPCHK(hipGetLastError());
        }
    }
    D.ranges.retried = T.retried;
    if (T.n_data) {
        set_err("reads: " + std::to_string(T.n_data) + " met a packet that does not decode as the index says" + (sc ? " or as its checksum says" : ""));
        return ZZ_E_DATA;
    }
    if (T.n_unsupported) { set_err("reads: " + std::to_string(T.n_unsupported) + " need more than one batch of packets: use zz_decode_range_device"); return ZZ_E_UNSUPPORTED; }
    if (T.n_arg) { set_err("reads: " + std::to_string(T.n_arg) + " start behind the index's last packet or overflow"); return ZZ_E_ARG; }
    if (T.n_nospace) { set_err("reads: " + std::to_string(T.n_nospace) + " do not fit their destinations"); return ZZ_E_NOSPACE; }
    return ZZ_OK;
}

extern "C" int zz_decode_ranges_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint32_t P,
                                       const uint64_t* d_index, uint64_t entries,
                                       uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                       void* const* d_dsts, const uint64_t* d_caps,
                                       uint64_t* d_out_lens, int32_t* d_status, void* hip_stream)
{
    return dec_ranges(c, d_src_v, src_len, format, P, d_index, entries, nullptr, nranges, d_firsts, d_nbytes, d_dsts, d_caps,
                      d_out_lens, d_status, hip_stream);
}
extern "C" int zz_decode_ranges_checked_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, uint32_t P,
                                               const uint64_t* d_index, uint64_t entries, const uint32_t* d_cks, uint64_t total_len,
                                               uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                               void* const* d_dsts, const uint64_t* d_caps,
                                               uint64_t* d_out_lens, int32_t* d_status, void* hip_stream)
{
    const dec_sidecar sc{ d_cks, total_len, zi_sidecar_kind(format), format };
    return dec_ranges(c, d_src_v, src_len, format, P, d_index, entries, &sc, nranges, d_firsts, d_nbytes, d_dsts, d_caps,
                      d_out_lens, d_status, hip_stream);
}

// The sidecar of d_data[0, n): zz_checksum.h's per-packet partials, then their public values (zz_inflate_check.h). Stateless.
extern "C" int zz_packet_checksums_device(zz_ctx* c, const void* d_data, uint64_t n, uint32_t P, int format,
                                          uint32_t* d_cks, uint64_t max_entries, uint64_t* entries, void* hip_stream)
{
    if (!c || !entries || !d_cks || (!d_data && n)) { set_err("null argument"); return ZZ_E_ARG; }
    if (!dec_packet_ok(P, 1) || !dec_format_ok(format)) return ZZ_E_ARG;
    const uint64_t npk = zi_sidecar_entries(n, P);
    if (npk > 0x7fffffffull) { set_err("at most 2^31 - 1 packets"); return ZZ_E_ARG; }
    *entries = npk;
    if (max_entries < npk) { set_err("checksum buffer too small"); return ZZ_E_NOSPACE; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = c->dec.side.grow(npk)) return rc;
    zz_packet_params pp = {};
    pp.src = (const uint8_t*)d_data; pp.n = n; pp.packet_size = P; pp.npk = (uint32_t)npk; pp.cks_kind = zi_sidecar_kind(format); pp.cks = c->dec.side;
    launch_cks_partials(pp, 16384, st);
    hipLaunchKernelGGL(k_cks_publish, dim3((uint32_t)((npk + 255) / 256)), dim3(256), 0, st, c->dec.side.p, (uint32_t)npk, P, n, pp.cks_kind, d_cks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

extern "C" int zz_ctx_last_decode_ranges_stats(const zz_ctx* c, uint64_t* packets, uint32_t* attempts, uint64_t* retried_ranges,
                                               uint32_t* waves)
{
    if (!c) { set_err("null context"); return ZZ_E_ARG; }
    if (packets) *packets = c->dec.ranges.packets;
    if (attempts) *attempts = c->dec.ranges.attempts;
    if (retried_ranges) *retried_ranges = c->dec.ranges.retried;
    if (waves) *waves = c->dec.ranges.waves;
    return ZZ_OK;
}

// The reference's sequential whole-buffer stream (threaded=false, zzflate.cpp:84-95) on the device. Level 0 is
// parallel (stored blocks of 65535 bytes have known places); level 1 is a chain of fixed-Huffman blocks whose lengths
// follow from the room in the output buffer (encoder.cpp:331-337: ONE block when the destination is roomy), levels
// 2,3 a chain of dynamic blocks, each chain produced by a single wavefront (k_stream_l1 / k_stream_l2) -- a
// compatibility mode, bit-identical to the reference, not a fast one.
//   chunked == false: ZzFlateEncode's caller-owned buffer of `cap` bytes (zzflate.cpp:225-242);
//   chunked == true : ZzFlateEncodeToCallback's library-owned chunks of 1,000,000 bytes (zzflate.cpp:197-222,
//                     outputbitstream.h:171-201); *chunk_sizes receives the byte counts the callback would see between the
//                     header call and the trailer call, `cap` only has to hold the stream.
static int encode_stream(zz_ctx* c, const uint8_t* d_src, uint64_t n, uint8_t* d_dst, uint64_t cap, int format, int level,
                         bool chunked, std::vector<uint64_t>* chunk_sizes, hipStream_t st, zz_result* host_res)
{
    if (call_pending(c)) return ZZ_E_ARG;
    begin_encode_call(c);
    if (level < 0 || level > 3) { set_err("level must be 0..3 (zzflate.cpp:201,230)"); return ZZ_E_LEVEL; }
    if (!d_dst || (!d_src && n)) { set_err("null buffer"); return ZZ_E_ARG; }
    if (chunk_sizes) chunk_sizes->clear();
    if (n == 0) {
        int rc = encode_common(c, d_src, 0, 0, true, d_dst, cap, format, cks_kind_for(format), true, level, ZZ_DEFAULT_PACKET, st, host_res);
        if (!rc && chunk_sizes && host_res->stream_bytes) chunk_sizes->push_back(host_res->stream_bytes);
        return rc;
    }
    if (n >= (1ull << 31)) { set_err("sequential stream: input must be < 2 GiB (the reference funnels lengths through int)"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const int hl = header_len(format), tl = trailer_len(format);
    if (cap < (uint64_t)hl) { set_err("destination smaller than the container header"); return ZZ_E_NOSPACE; }
    const int cks_kind = cks_kind_for(format);
    HIPCHK(hipMemsetAsync(c->d_res, 0, sizeof(zz_result), st));
    HIPCHK(hipMemsetAsync(c->d_cks_total, 0, sizeof(zz_cks_total), st));
    HIPCHK(hipMemsetAsync(c->d_err, 0, 4 * sizeof(uint32_t), st));
    zz_packet_params pp;
    memset(&pp, 0, sizeof pp);
    pp.src = d_src; pp.n = n; pp.halo = 0; pp.last_is_final = 1; pp.err = c->d_err; pp.prof = c->d_prof; pp.tail = c->d_tail;
    std::vector<uint64_t> log;          // (bytes stored, length asked for) per EnsureOutputLength call, chunked form
    uint32_t log_cap = 0;
    if (level == 0) {
        const uint32_t B = 0xFFFF;                                     // encoder.cpp:484
        const uint32_t npk = (uint32_t)((n + B - 1) / B);
        int rc = ensure_workspace(c, 0, npk, 0);
        if (rc) return rc;
        const uint64_t total = (uint64_t)(npk - 1) * (B + 5) + 5 + (n - (uint64_t)(npk - 1) * B);
        if ((uint64_t)hl + total + tl > cap) { set_err("destination too small"); return ZZ_E_NOSPACE; }
        pp.packet_size = B; pp.npk = npk; pp.cks_kind = cks_kind; pp.sizes = c->sizes; pp.cks = c->cks;
        if (cks_kind == ZZ_CKS_CRC) {                                  // (Adler partials are k_encode_l0's own)
            launch_cks_partials(pp, 0, st);
            pp.cks_kind = ZZ_CKS_NONE;
        }
        zz_l0_params q; q.pk = pp; q.dst = d_dst + hl; q.stream_mode = 1;
        hipLaunchKernelGGL(k_encode_l0, dim3(npk < 16384 ? npk : 16384), dim3(256), 0, st, q);
        hipLaunchKernelGGL(k_put_small, dim3(1), dim3(1), 0, st, (uint8_t*)nullptr, 0ull, 0u, c->d_res, total);
        if (chunked && chunk_sizes)                                     // WriteUncompressedBlock asks for 6 + length (encoder.cpp:488)
            for (uint32_t k = 0; k < npk; ++k) {
                log.push_back((uint64_t)k * (B + 5));
                log.push_back(6 + (k + 1 < npk ? (uint64_t)B : n - (uint64_t)(npk - 1) * B));
            }
    } else {
        // worst cases. Level 1: nine bits per byte plus ten per block; blocks of the chunked form hold at least
        // (2^18 - 1) * 8 / 9 - 8 bytes each, and a caller-owned buffer is never overrun (the block lengths see to it).
        // Level >= 2: every block falls back to stored blocks of <= 65535 bytes.
        const uint64_t avail = cap - hl;
        uint64_t bound = level == 1 ? ((uint64_t)9 * n + 17) / 8 + n / 65536 + 128 : n + (n / 65535 + 2) * 5 + (n / 400000 + 2) * 8 + 64;
        if (level == 1 && !chunked && avail + 64 < bound) bound = avail + 64;
        const uint32_t P = 32768, npk_c = (uint32_t)((n + P - 1) / P);   // checksum chunks
        int rc = ensure_workspace(c, 0, npk_c, 0);
        if (rc) return rc;
        if ((rc = c->slots.grow(bound))) return rc;
        zz_stream_ctl ctl;
        memset(&ctl, 0, sizeof ctl);
        ctl.cap = avail; ctl.chunked = chunked ? 1 : 0; ctl.truncated = c->d_err + 1; ctl.log_n = c->d_err + 2;
        if (chunked) {
            log_cap = (uint32_t)(n / 32768 + 64);                        // far more than the blocks a stream can have
            if ((rc = c->d_log.grow((uint64_t)log_cap * 2))) return rc;
            ctl.log = c->d_log; ctl.log_cap = log_cap;
        }
        pp.packet_size = P; pp.npk = npk_c; pp.cks_kind = cks_kind; pp.cks = c->cks; pp.sizes = c->sizes;
        launch_cks_partials(pp, 4096, st);
        zz_packet_params ps = pp;
        ps.npk = 1; ps.slots = c->slots; ps.slot_stride = (uint32_t)(bound > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : bound); ps.cks_kind = ZZ_CKS_NONE;
        if (level >= 2 && (rc = c->l2_scratch.grow(ZZ_ST_SCRATCH_BYTES))) return rc;
        if (c->timing) HIPCHK(hipEventRecord(c->ev0, st));
        if (level == 1) hipLaunchKernelGGL(k_stream_l1, dim3(1), dim3(ZZ_WAVE), 0, st, ps, ctl);
        else { zz_st_params q; q.pk = ps; q.scratch = c->l2_scratch; q.ctl = ctl; hipLaunchKernelGGL(k_stream_l2, dim3(1), dim3(ZZ_WAVE), 0, st, q); }
        if (c->timing) { HIPCHK(hipEventRecord(c->ev1, st)); c->have_time = true; }
        hipLaunchKernelGGL(k_copy_stream, dim3(1024), dim3(256), 0, st, c->slots, c->sizes, d_dst + hl,
                           cap >= (uint64_t)(hl + tl) ? cap - hl - tl : 0, c->d_res);
    }
    launch_cks_fold(c, pp, cks_kind, st);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1), 0, st, d_dst, cap, format, c->d_cks_total, n, c->d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_res, c->d_res, sizeof(zz_result), hipMemcpyDeviceToHost, st));
    // (into pinned memory: an asynchronous copy into pageable memory is staged by the runtime and makes concurrent callers on
    // other streams take turns)
    HIPCHK(hipMemcpyAsync(c->h_err, c->d_err, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint32_t kerr[4] = { c->h_err[0], c->h_err[1], c->h_err[2], c->h_err[3] };
    *host_res = *c->h_res;
    if (kerr[0]) { set_err("internal: output slot overflow"); return ZZ_E_NOSPACE; }
    if (kerr[1]) {
        set_err("destination too small: the reference's level-1 stream stops early here (encoder.cpp:331-337,546-548)");
        return ZZ_E_NOSPACE;
    }
    if (host_res->err) { set_err("destination too small for the compressed stream"); return ZZ_E_NOSPACE; }
    if (chunked && chunk_sizes) {
        if (level != 0) {
            const uint32_t nlog = kerr[2];
            if (nlog > log_cap) { set_err("internal: chunk log overflow"); return ZZ_E_HIP; }
            log.resize((size_t)nlog * 2);
            if (nlog) HIPCHK(hipMemcpy(log.data(), c->d_log, (size_t)nlog * 16, hipMemcpyDeviceToHost));
        }
        // replay EnsureOutputLength (outputbitstream.h:171-190) over the log: a chunk starts where the rule opens one
        zz_chunker ck = { 0, 0 };
        std::vector<uint64_t> starts;
        for (size_t k = 0; k + 1 < log.size(); k += 2) {
            bool opened;
            const int64_t room = zz_chunk_ensure(ck, log[k], (int64_t)log[k + 1], &opened);
            if (level >= 2 && !opened && room < (int64_t)log[k + 1]) {
                // a dynamic block that needs more than the > 2^18 bytes still free: the reference gives up here
                // (encoder.cpp:277-278) and leaves an undecodable stream; the block is in ours, so it gets a chunk of
                // its own. (At level 1 the length asked for is only a wish: the block is cut to what fits.)
                ck.chunk_start = log[k]; ck.nchunks++; opened = true;
            }
            if (opened) starts.push_back(log[k]);
        }
        for (size_t k = 0; k < starts.size(); ++k) {
            const uint64_t e = k + 1 < starts.size() ? starts[k + 1] : host_res->stream_bytes;
            chunk_sizes->push_back(e - starts[k]);
        }
    }
    return ZZ_OK;
}

// The reference's OWN threaded=true split (zzflate.cpp:67-78 divideInRanges, :97-155): `count` ranges of ceil(n / count) bytes
// -- count is std::thread::hardware_concurrency() there, the caller's choice here --, every range a fresh encoder, joined in
// order. Packet mode replaces this split by fixed ranges of <= 32 KiB because a GPU wants thousands of ranges;
// this entry point reproduces the reference's bytes for a given count: one WAVEFRONT per range (k_stream_l2: a range is one
// dependency chain, and longer than the packet kernels' 16-bit positions allow), so it is a compatibility mode like the
// sequential stream. Levels 0, 2, 3: at level 1 the reference's threaded stream is invalid (the block
// lengths follow from the room, destLen / count per range, and the joined stream does not inflate), so there is nothing to equal.
// every range of the reference's split starts inside the input: (count - 1) * ceil(n / count) < n
static bool ranges_split_ok(uint64_t n, uint32_t count)
{
    if (count == 0) return false;
    const uint64_t step = (n + count - 1) / count;
    return (uint64_t)(count - 1) * step < n;
}
static int encode_ranges(zz_ctx* c, const uint8_t* d_src, uint64_t n, uint8_t* d_dst, uint64_t cap, int format, int level,
                         uint32_t count, hipStream_t st, zz_result* host_res)
{
    if (call_pending(c)) return ZZ_E_ARG;
    begin_encode_call(c);
    if (count == 0 || count > 4096) { set_err("ranges: count must be 1..4096"); return ZZ_E_ARG; }
    if (level == 1) { set_err("ranges: the reference's threaded level-1 stream is invalid (block lengths follow from destLen / count); use packet mode"); return ZZ_E_LEVEL; }
    if (n < 100ull * count)                                               // zzflate.cpp:84: the single encoder
        return encode_stream(c, d_src, n, d_dst, cap, format, level, false, nullptr, st, host_res);
    if (level < 0 || level > 3) { set_err("level must be 0..3 (zzflate.cpp:201,230)"); return ZZ_E_LEVEL; }
    if (!d_dst || !d_src) { set_err("null buffer"); return ZZ_E_ARG; }
    if (n >= (1ull << 31)) { set_err("ranges: input must be < 2 GiB (the reference funnels lengths through int)"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const int hl = header_len(format), tl = trailer_len(format);
    if (cap < (uint64_t)hl) { set_err("destination smaller than the container header"); return ZZ_E_NOSPACE; }
    const int cks_kind = cks_kind_for(format);
    const uint64_t step = (n + count - 1) / count;                        // zzflate.cpp:70
    // divideInRanges (zzflate.cpp:67-78) puts boundary i at step * i and only the last one at n: with count near sqrt(n) or
    // above, the trailing boundaries lie at or past n (the reference then reads past its input and joins
    // a stream that does not inflate -- undefined behaviour, nothing to equal). Refused here, before anything is launched.
    if (!ranges_split_ok(n, count)) {
        set_err("ranges: count too large for this input: (count - 1) * ceil(n / count) must be < n (zzflate.cpp:67-78 would cut ranges past the input's end)");
        return ZZ_E_ARG;
    }
    HIPCHK(hipMemsetAsync(c->d_res, 0, sizeof(zz_result), st));
    HIPCHK(hipMemsetAsync(c->d_cks_total, 0, sizeof(zz_cks_total), st));
    HIPCHK(hipMemsetAsync(c->d_err, 0, 4 * sizeof(uint32_t), st));
    const uint32_t P = 32768, npk_c = (uint32_t)((n + P - 1) / P);         // checksum chunks
    int rc = ensure_workspace(c, 0, npk_c > count ? npk_c : count, 0);
    if (rc) return rc;
    zz_packet_params pp;
    memset(&pp, 0, sizeof pp);
    pp.src = d_src; pp.n = n; pp.halo = 0; pp.last_is_final = 1; pp.err = c->d_err; pp.prof = c->d_prof; pp.tail = c->d_tail;
    pp.packet_size = P; pp.npk = npk_c; pp.cks_kind = cks_kind; pp.cks = c->cks; pp.sizes = c->sizes;
    launch_cks_partials(pp, 4096, st);
    if (level == 0) {
        const uint64_t total = (uint64_t)(count - 1) * l0_range_bytes(step, false) + l0_range_bytes(n - (uint64_t)(count - 1) * step, true);
        if ((uint64_t)hl + total + tl > cap) { set_err("destination too small"); return ZZ_E_NOSPACE; }
        hipLaunchKernelGGL(k_ranges_l0, dim3(count), dim3(256), 0, st, d_src, n, step, d_dst + hl);
        hipLaunchKernelGGL(k_put_small, dim3(1), dim3(1), 0, st, (uint8_t*)nullptr, 0ull, 0u, c->d_res, total);
    } else {
        // per range: every block may fall back to stored blocks of <= 65535 bytes, plus the closing stored byte
        const uint64_t bound = (step + (step / 65535 + 2) * 5 + (step / 400000 + 2) * 8 + 64 + 15) & ~15ull;
        if (bound > 0xFFFFFFF0ull) { set_err("ranges: range too large"); return ZZ_E_ARG; }
        if ((rc = c->slots.grow(bound * count))) return rc;
        if ((rc = c->l2_scratch.grow((uint64_t)ZZ_ST_SCRATCH_BYTES * count))) return rc;
        zz_st_params q;
        memset(&q, 0, sizeof q);
        q.pk = pp; q.pk.npk = count; q.pk.slots = c->slots; q.pk.slot_stride = (uint32_t)bound; q.pk.cks_kind = ZZ_CKS_NONE;
        q.scratch = c->l2_scratch; q.range_step = step;
        q.ctl.cap = ~0ull;
        if (c->timing) HIPCHK(hipEventRecord(c->ev0, st));
        hipLaunchKernelGGL(k_stream_l2, dim3(count), dim3(ZZ_WAVE), 0, st, q);
        if (c->timing) { HIPCHK(hipEventRecord(c->ev1, st)); c->have_time = true; }
        hipLaunchKernelGGL(k_scan_sizes, dim3(1), dim3(ZZ_SCAN_THREADS), 0, st, c->sizes, count, c->offsets, c->d_res);
        hipLaunchKernelGGL(k_compact, dim3(count), dim3(256), 0, st, c->slots, (uint32_t)bound, c->sizes, c->offsets, count,
                           d_dst + hl, cap >= (uint64_t)(hl + tl) ? cap - hl - tl : 0, c->d_res);
    }
    launch_cks_fold(c, pp, cks_kind, st);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1), 0, st, d_dst, cap, format, c->d_cks_total, n, c->d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_res, c->d_res, sizeof(zz_result), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c->h_err, c->d_err, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *host_res = *c->h_res;
    if (c->h_err[0]) { set_err("internal: output slot overflow"); return ZZ_E_NOSPACE; }
    if (host_res->err) { set_err("destination too small for the compressed stream"); return ZZ_E_NOSPACE; }
    return ZZ_OK;
}

extern "C" int zz_encode_ranges_device(zz_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                                       int format, int level, uint32_t count, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    if (format < 0 || format > 2) format = ZZ_DEFLATE;
    zz_result r;
    int rc = encode_ranges(c, (const uint8_t*)d_src, n, (uint8_t*)d_dst, cap, format, level, count, (hipStream_t)hip_stream, &r);
    if (rc) return rc;
    *out_len = r.total_bytes;
    return ZZ_OK;
}

extern "C" int zz_encode_stream_device(zz_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                                       int format, int level, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c || !out_len) { set_err("null ctx/out_len"); return ZZ_E_ARG; }
    if (format < 0 || format > 2) format = ZZ_DEFLATE;
    zz_result r;
    int rc = encode_stream(c, (const uint8_t*)d_src, n, (uint8_t*)d_dst, cap, format, level, false, nullptr, (hipStream_t)hip_stream, &r);
    if (rc) return rc;
    *out_len = r.total_bytes;
    return ZZ_OK;
}

extern "C" int zz_encode_stream_chunks_device(zz_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                                              int format, int level, uint64_t* chunk_sizes, uint32_t max_chunks,
                                              uint32_t* nchunks, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (nchunks) *nchunks = 0;
    if (!c || !out_len) { set_err("null ctx/out_len"); return ZZ_E_ARG; }
    if (format < 0 || format > 2) format = ZZ_DEFLATE;
    zz_result r;
    std::vector<uint64_t> sizes;
    int rc = encode_stream(c, (const uint8_t*)d_src, n, (uint8_t*)d_dst, cap, format, level, true, &sizes, (hipStream_t)hip_stream, &r);
    if (rc) return rc;
    *out_len = r.total_bytes;
    if (nchunks) *nchunks = (uint32_t)sizes.size();
    if (chunk_sizes) for (size_t k = 0; k < sizes.size() && k < max_chunks; ++k) chunk_sizes[k] = sizes[k];
    return ZZ_OK;
}


extern "C" int zz_encode_device(zz_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                                int format, int level, uint32_t P, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c || !out_len) { set_err("null ctx/out_len"); return ZZ_E_ARG; }
    if (format < 0 || format > 2) format = ZZ_DEFLATE;   // zzflate.cpp:39-48 default branch
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    zz_result r;
    int rc = encode_common(c, (const uint8_t*)d_src, n, 0, true, (uint8_t*)d_dst, cap, format, cks_kind_for(format),
                           true, level, P, (hipStream_t)hip_stream, &r);
    if (rc) return rc;
    *out_len = r.total_bytes;
    return ZZ_OK;
}

// The same call in two halves, so that several calls -- on several contexts, each with its own stream -- can be in flight:
// the next call's encode kernel then fills the CUs the previous one's last packets leave idle, and runs under its
// compaction, checksum fold and result copy. zz_encode_device_async enqueues everything and returns; zz_encode_finish
// waits for it and hands out the length (or the error). One call per context at a time; source, destination and the
// stream must stay alive in between.
extern "C" int zz_encode_device_async(zz_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, int format, int level,
                                      uint32_t P, void* hip_stream)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (format < 0 || format > 2) format = ZZ_DEFLATE;
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    return encode_common(c, (const uint8_t*)d_src, n, 0, true, (uint8_t*)d_dst, cap, format, cks_kind_for(format), true, level, P,
                         (hipStream_t)hip_stream, nullptr);
}
extern "C" int zz_encode_finish(zz_ctx* c, uint64_t* out_len)
{
    if (out_len) *out_len = ~0ull;
    if (!c || !out_len) { set_err("null ctx/out_len"); return ZZ_E_ARG; }
    zz_result r;
    int rc = encode_finish(c, &r);
    if (rc) return rc;
    *out_len = r.total_bytes;
    return ZZ_OK;
}

extern "C" int zz_encode_shard_device(zz_ctx* c, const void* d_src, uint64_t n, uint64_t halo, int is_last, void* d_dst,
                                      uint64_t cap, uint64_t* out_len, uint32_t* cks, int checksum, int level,
                                      uint32_t P, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c || !out_len) { set_err("null ctx/out_len"); return ZZ_E_ARG; }
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    zz_result r;
    int rc = encode_common(c, (const uint8_t*)d_src, n, halo, is_last != 0, (uint8_t*)d_dst, cap, ZZ_DEFLATE,
                           cks_kind_for(checksum), false, level, P, (hipStream_t)hip_stream, &r);
    if (rc) return rc;
    *out_len = r.stream_bytes;
    if (cks) *cks = checksum == ZZ_ZLIB ? ((r.cks_b << 16) | r.cks_a) : r.cks_a;
    return ZZ_OK;
}

// The shard call in two halves (as zz_encode_device_async / zz_encode_finish): a rank can enqueue the next step's shard
// before it has exchanged the previous one's size and checksum with its peers, so the GPU never waits for the host.
extern "C" int zz_encode_shard_device_async(zz_ctx* c, const void* d_src, uint64_t n, uint64_t halo, int is_last, void* d_dst,
                                            uint64_t cap, int checksum, int level, uint32_t P, void* hip_stream)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    return encode_common(c, (const uint8_t*)d_src, n, halo, is_last != 0, (uint8_t*)d_dst, cap, ZZ_DEFLATE, cks_kind_for(checksum),
                         false, level, P, (hipStream_t)hip_stream, nullptr);
}
extern "C" int zz_encode_shard_finish(zz_ctx* c, uint64_t* out_len, uint32_t* cks, int checksum)
{
    if (out_len) *out_len = ~0ull;
    if (!c || !out_len) { set_err("null ctx/out_len"); return ZZ_E_ARG; }
    zz_result r;
    int rc = encode_finish(c, &r);
    if (rc) return rc;
    *out_len = r.stream_bytes;
    if (cks) *cks = checksum == ZZ_ZLIB ? ((r.cks_b << 16) | r.cks_a) : r.cks_a;
    return ZZ_OK;
}

// ---- many independent streams in one call (zz_batch.h) --------------------------------------------------------------------
// What a batch or a member file runs at: the level of its frame (slots, strides, the join), and for the extended levels the chain
// depth and the window they bring.
struct batch_level { int level, xdepth; uint32_t warm; };
// Batches and members accept a level. Without the call's own extended switch: as ever -- cold packets of levels 0..3, and a context with a
// warm window or the extended levels on is refused. With it: the context's extended switch does not matter (it stays the single-stream
// calls'), a warm window still refuses, levels 0..3 are the same calls, and levels 4..6 run in level 2's frame where the device's
// LDS-order verdict is positive (as zz_ctx_set_extended_levels asks).
static int accept_batch_level(zz_ctx* c, int level, bool extended, const char* what, batch_level* out)
{
    if (c->warm || (c->extended && !extended)) {
        set_err(std::string(what) + " take cold packets of levels 0..3: switch the warm window and the extended levels off on this context");
        return ZZ_E_UNSUPPORTED;
    }
    out->level = level; out->xdepth = 0; out->warm = 0;
    if (extended && level >= 4 && level <= 6) {
        if (!lds_order_ok(c->device)) {
            set_err("extended levels refused: this device's LDS does not serve equal addresses in lane order (probe k_lds_order_probe failed)");
            return ZZ_E_UNSUPPORTED;
        }
        out->xdepth = level == 4 ? 2 : level == 5 ? 4 : 8;
        out->warm = level == 4 ? 8192u : 32768u;
        out->level = 2;
        return ZZ_OK;
    }
    if (level < 0 || level > 3) {
        set_err(extended ? "level must be 0..6" : "level must be 0..3 (zzflate.cpp:201,230)");
        return ZZ_E_LEVEL;
    }
    return ZZ_OK;
}
static int encode_batch(zz_ctx* c, uint32_t nitems, const uint8_t* const* d_srcs, const uint64_t* d_ns, uint8_t* const* d_dsts,
                        const uint64_t* d_caps, uint64_t* d_out_lens, int format, batch_level lv, uint32_t P, hipStream_t st, bool one_parser)
{
    const int level = lv.level;
    const int cks_kind = cks_kind_for(format);
    begin_encode_call(c);
    if (int rc = ensure_items(c, (uint64_t)nitems + 1)) return rc;
    if (int rc = c->bat.d_tot.grow(1)) return rc;
    if (int rc = c->bat.h_tot.grow(1)) return rc;
    HIPCHK(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), st));
    // the plan; its two totals are the one thing the host reads before the launches (grid and workspace sizes)
    hipLaunchKernelGGL(k_batch_plan, dim3(1), dim3(ZZ_SCAN_THREADS), 0, st, d_ns, nitems, P, level, c->bat.first, c->bat.slotbase, c->bat.d_tot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->bat.h_tot, c->bat.d_tot, sizeof(zz_batch_totals), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t npk64 = c->bat.h_tot->npk, slot_bytes = c->bat.h_tot->slot_bytes + 256;   // (+ room behind the last slot)
    if (npk64 > 0x7FFFFFFFull) { set_err("too many packets for one call"); return ZZ_E_ARG; }
    const uint32_t npk = (uint32_t)npk64;
    // the same kernel choice as a single call, and the same run-time check behind the LDS-order verdict
    const launch_plan plan = plan_launch(c, level, lv.warm, lv.xdepth, one_parser);     // (the extended levels: no two-parser kernel, no order check, no rerun)
    if (npk) if (int rc = ensure_batch_workspace(c, level, npk, slot_bytes, P, lv.xdepth)) return rc;
    zz_batch_map M;
    M.desc = c->bat.desc; M.srcs = d_srcs; M.ns = d_ns; M.first = c->bat.first; M.tails = c->bat.tails; M.npk = npk; M.level = level;
    if (npk) {
        hipLaunchKernelGGL(k_batch_desc, dim3((npk + 255) / 256), dim3(256), 0, st, c->bat.first, nitems, npk, P, level, c->bat.slotbase, c->bat.desc);
        if (level >= 1)
            hipLaunchKernelGGL(k_batch_tails, dim3(nitems < 65536 ? nitems : 65536), dim3(128), 0, st, d_srcs, d_ns, nitems, c->bat.tails);
        zz_packet_params pp = packet_params(c, npk, P, cks_kind, plan);
        pp.warm = lv.warm;
        if (int rc = launch_packet_encoders(c, pp, &M, level, lv.xdepth, plan, st)) return rc;
        if (level == 0) {
            zz_l0_batch_params q; q.pk = pp; q.dsts = d_dsts; q.caps = d_caps; q.format = format;
            hipLaunchKernelGGL(k_encode_l0_batch, dim3(npk < 16384 ? npk : 16384), dim3(256), 0, st, q, M);
        }
        if (int rc = end_packet_encoders(c, level, npk, st)) return rc;
    }
    zz_batch_join J;
    J.map = M; J.sizes = c->sizes; J.offsets = c->offsets; J.cks = c->cks; J.slots = c->slots; J.dsts = d_dsts; J.caps = d_caps;
    J.out_lens = d_out_lens; J.totals = c->bat.d_tot; J.nitems = nitems; J.packet_size = P; J.format = format; J.cks_kind = cks_kind;
    J.level = level;
    const uint32_t per_fin = ZZ_BATCH_FIN_THREADS / ZZ_WAVE, gf = (nitems + per_fin - 1) / per_fin;
    hipLaunchKernelGGL(k_batch_finalize, dim3(gf < 65536 ? gf : 65536), dim3(ZZ_BATCH_FIN_THREADS), 0, st, J);
    if (npk && level != 0) {
        const uint32_t per_cp = ZZ_BATCH_COMPACT_THREADS / ZZ_WAVE, gc = (npk + per_cp - 1) / per_cp;
        hipLaunchKernelGGL(k_batch_compact, dim3(gc < 65536 ? gc : 65536), dim3(ZZ_BATCH_COMPACT_THREADS), 0, st, J);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->bat.h_tot, c->bat.d_tot, sizeof(zz_batch_totals), hipMemcpyDeviceToHost, st));
    const int ew = finish_err_word(c, plan.order_checked, st);
    if (ew == ERR_RERUN)                 // as encode_finish: the whole batch runs again on the one-parser kernels
        return encode_batch(c, nitems, d_srcs, d_ns, d_dsts, d_caps, d_out_lens, format, lv, P, st, true);
    if (ew) return ew;
    if (c->bat.h_tot->nospace) {
        set_err(std::to_string(c->bat.h_tot->nospace) + " of " + std::to_string(nitems) + " items did not fit their destination");
        return ZZ_E_NOSPACE;
    }
    return ZZ_OK;
}

extern "C" int zz_encode_batch_flags_device(zz_ctx* c, uint64_t nitems, const void* const* d_srcs, const uint64_t* d_ns,
                                            void* const* d_dsts, const uint64_t* d_caps, uint64_t* d_out_lens,
                                            int format, int level, uint32_t P, int flags, void* hip_stream)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (flags & ~ZZ_BATCH_EXTENDED) { set_err("unknown flags"); return ZZ_E_ARG; }
    if (nitems == 0) return ZZ_OK;
    if (!d_srcs || !d_ns || !d_dsts || !d_caps || !d_out_lens) { set_err("null array"); return ZZ_E_ARG; }
    if (nitems > 0x7FFFFFFFull) { set_err("too many items for one call"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    batch_level lv;
    if (int rc = accept_batch_level(c, level, (flags & ZZ_BATCH_EXTENDED) != 0, "batches", &lv)) return rc;
    if (format < 0 || format > 2) format = ZZ_DEFLATE;   // zzflate.cpp:39-48 default branch
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    if (P > ZZ_MAX_PACKET_SIZE) { set_err("packet size must be 1..32768"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return encode_batch(c, (uint32_t)nitems, (const uint8_t* const*)d_srcs, d_ns, (uint8_t* const*)d_dsts, d_caps, d_out_lens, format,
                        lv, P, (hipStream_t)hip_stream, false);
}
extern "C" int zz_encode_batch_device(zz_ctx* c, uint64_t nitems, const void* const* d_srcs, const uint64_t* d_ns,
                                      void* const* d_dsts, const uint64_t* d_caps, uint64_t* d_out_lens,
                                      int format, int level, uint32_t P, void* hip_stream)
{
    return zz_encode_batch_flags_device(c, nitems, d_srcs, d_ns, d_dsts, d_caps, d_out_lens, format, level, P, 0, hip_stream);
}

// ---- one buffer to a blocked gzip (BGZF) file (zz_members_write.h) ----------------------------------------------------------
// bytes of the file when every member takes its stored form: the bound, and what mw_geometry_ok keeps below 65,536 per member
static uint64_t members_stored_bytes(uint64_t n, uint32_t B, uint32_t P)
{
    if (n == 0) return 0;
    const uint64_t m = (n + B - 1) / B;
    return (m - 1) * (ZZ_MW_HEADER + l0_item_bytes(B, P) + ZZ_MW_TRAILER) + ZZ_MW_HEADER + l0_item_bytes(n - (m - 1) * B, P) + ZZ_MW_TRAILER;
}
static bool members_sizes(uint32_t& B, uint32_t& P)
{
    if (B == 0) B = ZZ_MEMBERS_BLOCK;
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    return P <= ZZ_MAX_PACKET_SIZE && mw_geometry_ok(B, P);
}
extern "C" uint64_t zz_encode_members_bound(uint64_t n, uint32_t B, uint32_t P, int flags)
{
    if (!members_sizes(B, P)) return ~0ull;
    return members_stored_bytes(n, B, P) + ((flags & ZZ_MEMBERS_NO_EOF) ? 0 : ZZ_MW_EOF);
}
extern "C" int zz_members_header(uint32_t member_bytes, uint8_t out[18])
{
    if (!out || member_bytes == 0 || member_bytes > ZZ_MW_MAX_MEMBER) { set_err("a member has 1..65536 bytes"); return ZZ_E_ARG; }
    mw_header(member_bytes, out);
    return ZZ_MW_HEADER;
}

static int encode_members(zz_ctx* c, const uint8_t* d_src, uint64_t n, uint8_t* d_dst, uint64_t cap, uint64_t* out_len, batch_level lv,
                          uint32_t B, uint32_t P, int flags, uint64_t* d_member_offsets, hipStream_t st, bool one_parser)
{
    auto& W = c->mw;
    const int level = lv.level;
    begin_encode_call(c);
    // members, packets and slot bytes in closed form: the host reads nothing back before the launches
    const uint32_t m = (uint32_t)((n + B - 1) / B), ppm = (B + P - 1) / P;
    const uint32_t last = m ? (uint32_t)(n - (uint64_t)(m - 1) * B) : 0;
    const uint32_t npk = m ? (m - 1) * ppm + (last + P - 1) / P : 0;
    const auto block_slots = [&](uint32_t len) -> uint64_t {
        const uint32_t k = (len + P - 1) / P;
        return level ? (uint64_t)(k - 1) * zz_slot_stride(level, P) + zz_slot_stride(level, len - (k - 1) * P) : 0;
    };
    const uint64_t full_slots = block_slots(B);
    const uint64_t slot_bytes = m ? (uint64_t)(m - 1) * full_slots + block_slots(last) + 256 : 0;     // (+ room behind the last slot)
    const uint64_t mm = (uint64_t)m + 1;
    if (int rc = ensure_items(c, mm)) return rc;
    if (int rc = W.srcs.grow(mm)) return rc;
    if (int rc = W.ns.grow(mm)) return rc;
    if (int rc = W.moff.grow(mm)) return rc;
    if (int rc = W.stored.grow(mm)) return rc;
    if (int rc = W.d_st.grow(1)) return rc;
    if (int rc = W.h_st.grow(1)) return rc;
    if (npk) if (int rc = ensure_batch_workspace(c, level, npk, level ? slot_bytes : 0, P, lv.xdepth)) return rc;      // (level 0 has no slots)
    HIPCHK(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), st));
    const launch_plan plan = plan_launch(c, level, lv.warm, lv.xdepth, one_parser);
    zz_mw_params Q;
    Q.src = d_src; Q.n = n; Q.dst = d_dst; Q.cap = cap; Q.B = B; Q.P = P; Q.members = m; Q.ppm = ppm;
    Q.eof = (flags & ZZ_MEMBERS_NO_EOF) ? 0 : ZZ_MW_EOF; Q.level = level; Q.full_slots = full_slots;
    Q.srcs = W.srcs; Q.ns = W.ns; Q.first = c->bat.first; Q.desc = c->bat.desc;
    Q.sizes = c->sizes; Q.offsets = c->offsets; Q.cks = c->cks; Q.slots = c->slots;
    Q.moff = W.moff; Q.stored = W.stored; Q.st = W.d_st; Q.user_offsets = d_member_offsets;
    if (npk) {
        hipLaunchKernelGGL(k_mw_items, dim3((m + 1 + 255) / 256), dim3(256), 0, st, Q);
        hipLaunchKernelGGL(k_mw_desc, dim3((npk + 255) / 256), dim3(256), 0, st, Q, npk);
        zz_batch_map M;
        M.desc = c->bat.desc; M.srcs = W.srcs; M.ns = W.ns; M.first = c->bat.first; M.tails = c->bat.tails; M.npk = npk; M.level = level;
        if (level >= 1)
            hipLaunchKernelGGL(k_batch_tails, dim3(m < 65536 ? m : 65536), dim3(128), 0, st, (const uint8_t* const*)W.srcs.p, (const uint64_t*)W.ns, m,
                               (uint8_t*)c->bat.tails);
        zz_packet_params pp = packet_params(c, npk, P, ZZ_CKS_CRC, plan);
        pp.warm = lv.warm;
        if (int rc = launch_packet_encoders(c, pp, &M, level, lv.xdepth, plan, st)) return rc;      // (level 0: the CRC pass alone; k_mw_stored writes the blocks)
        if (int rc = end_packet_encoders(c, level, npk, st)) return rc;
    }
    // the members' sizes and places, and the room check: nothing below stores a byte unless the file fits
    hipLaunchKernelGGL(k_mw_sizes, dim3(1), dim3(ZZ_SCAN_THREADS), 0, st, Q);
    const uint32_t per_fin = ZZ_MW_FIN_THREADS / ZZ_WAVE, gf = (m + per_fin - 1) / per_fin;
    hipLaunchKernelGGL(k_mw_finalize, dim3(gf < 65536 ? (gf ? gf : 1) : 65536), dim3(ZZ_MW_FIN_THREADS), 0, st, Q);
    if (npk && level != 0) {
        const uint32_t per_cp = ZZ_MW_COMPACT_THREADS / ZZ_WAVE, gc = (npk + per_cp - 1) / per_cp;
        hipLaunchKernelGGL(k_mw_compact, dim3(gc < 65536 ? gc : 65536), dim3(ZZ_MW_COMPACT_THREADS), 0, st, Q, npk);
    }
    if (npk) hipLaunchKernelGGL(k_mw_stored, dim3(npk < 16384 ? npk : 16384), dim3(256), 0, st, Q, npk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(W.h_st, W.d_st, sizeof(zz_mw_state), hipMemcpyDeviceToHost, st));
    const int ew = finish_err_word(c, plan.order_checked, st);
    if (ew == ERR_RERUN)                 // as encode_batch: the whole call runs again on the one-parser kernels
        return encode_members(c, d_src, n, d_dst, cap, out_len, lv, B, P, flags, d_member_offsets, st, true);
    if (ew) return ew;
    if (!W.h_st->fits) {
        set_err("the file (" + std::to_string(W.h_st->total + Q.eof) + " bytes) does not fit the destination");
        return ZZ_E_NOSPACE;
    }
    W.members = m; W.stored_members = W.h_st->stored;
    *out_len = W.h_st->total + Q.eof;
    return ZZ_OK;
}

extern "C" int zz_encode_members_device(zz_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t cap, uint64_t* out_len,
                                        int level, uint32_t block_size, uint32_t packet_size, int flags,
                                        uint64_t* d_member_offsets, uint64_t max_offsets, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    c->mw.members = 0; c->mw.stored_members = 0;
    if (!out_len) { set_err("null out_len"); return ZZ_E_ARG; }
    if (!d_src && n) { set_err("null source"); return ZZ_E_ARG; }
    if (!d_dst && cap) { set_err("null destination"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    batch_level lv;
    if (int rc = accept_batch_level(c, level, (flags & ZZ_MEMBERS_EXTENDED) != 0, "members", &lv)) return rc;
    uint32_t B = block_size, P = packet_size;
    if (!members_sizes(B, P)) {
        set_err("block size must be 1..65536, packet size 1..32768, and a block's stored member (26 bytes + its level-0 stream) at most 65536 bytes");
        return ZZ_E_ARG;
    }
    const uint64_t m = (n + B - 1) / B;
    if (m > 0x7FFFFFFFull || m * ((B + P - 1) / P) > 0x7FFFFFFFull) { set_err("too many members or packets for one call"); return ZZ_E_ARG; }
    if (d_member_offsets && max_offsets < m + 1) { set_err("the offsets array takes members + 1 entries"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return encode_members(c, (const uint8_t*)d_src, n, (uint8_t*)d_dst, cap, out_len, lv, B, P, flags, d_member_offsets,
                          (hipStream_t)hip_stream, false);
}
extern "C" int zz_ctx_last_encode_members_stats(const zz_ctx* c, uint64_t* members, uint64_t* stored_members)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (members) *members = c->mw.members;
    if (stored_members) *stored_members = c->mw.stored_members;
    return ZZ_OK;
}

// ---- a batch of independent streams back to their bytes (zz_inflate.h, k_inflate_items) ---------------------------------------
static_assert(ZI_ITEM_OK == ZZ_OK && ZI_ITEM_NOSPACE == ZZ_E_NOSPACE && ZI_ITEM_UNSUPPORTED == ZZ_E_UNSUPPORTED && ZI_ITEM_DATA == ZZ_E_DATA,
              "zi_item reports the C ABI's codes");
// k_inflate_items over q's items (its counters are the context's): returns when the two failure counters are in c->dec.items_host
static int dec_items(zz_ctx* c, zz_inf_items_params q, hipStream_t st)
{
    // workspace: the dealing counter and the two failure counters (and their pinned mirror)
    if (int rc = c->dec.items_ctr.grow(4)) return rc;
    if (int rc = c->dec.items_host.grow(2)) return rc;
    HIPCHK(hipMemsetAsync(c->dec.items_ctr, 0, 4 * sizeof(unsigned long long), st));
    q.fails = c->dec.items_ctr; q.next = (unsigned int*)(c->dec.items_ctr + 2);
    const uint64_t resident = 256ull * ZZ_INF_ITEM_WG_PER_CU;      // persistent wavefronts: what the CUs hold at once
    hipLaunchKernelGGL(k_inflate_items, dim3((uint32_t)(q.nitems < resident ? q.nitems : resident)), dim3(ZZ_INF_THREADS), 0, st, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->dec.items_host, c->dec.items_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}
// the members of a file as k_inflate_items' items (mem's five descriptor arrays), for zz_decode_members_device and the member reads
static int ensure_member_items(zz_ctx* c, uint64_t items)
{
    auto& M = c->dec.mem;
    if (int rc = M.srcs.grow(items)) return rc;
    if (int rc = M.dsts.grow(items)) return rc;
    if (int rc = M.src_lens.grow(items)) return rc;
    if (int rc = M.caps.grow(items)) return rc;
    return M.out_lens.grow(items);
}
static zz_inf_items_params member_items_params(zz_ctx* c, uint32_t nitems, int32_t* status)
{
    auto& M = c->dec.mem;
    zz_inf_items_params p;
    p.srcs = (const uint8_t* const*)M.srcs.p; p.src_lens = M.src_lens; p.dsts = (uint8_t* const*)M.dsts.p; p.caps = M.caps;
    p.out_lens = M.out_lens; p.status = status; p.nitems = nitems; p.format = ZZ_GZIP;
    return p;
}
extern "C" int zz_decode_batch_device(zz_ctx* c, uint64_t nitems, const void* const* d_srcs, const uint64_t* d_src_lens,
                                      void* const* d_dsts, const uint64_t* d_caps, uint64_t* d_out_lens, int32_t* d_status,
                                      int format, void* hip_stream)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (nitems == 0) return ZZ_OK;
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    if (call_pending(c)) return ZZ_E_ARG;
    if (!d_srcs || !d_src_lens || !d_dsts || !d_caps || !d_out_lens) { set_err("null array"); return ZZ_E_ARG; }
    if (nitems > 0x7FFFFFFFull) { set_err("too many items for one call"); return ZZ_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    zz_inf_items_params q;
    q.srcs = (const uint8_t* const*)d_srcs; q.src_lens = d_src_lens; q.dsts = (uint8_t* const*)d_dsts; q.caps = d_caps;
    q.out_lens = d_out_lens; q.status = d_status; q.nitems = (uint32_t)nitems; q.format = format;
    if (int rc = dec_items(c, q, st)) return rc;
    const unsigned long long bad = c->dec.items_host[0], nospace = c->dec.items_host[1];
    if (bad) {
        set_err(std::to_string(bad) + " of " + std::to_string(nitems) + " items are not valid streams of the requested format (or need a preset dictionary)" +
                (nospace ? ", " + std::to_string(nospace) + " did not fit their destination" : std::string()));
        return ZZ_E_DATA;
    }
    if (nospace) {
        set_err(std::to_string(nospace) + " of " + std::to_string(nitems) + " items did not fit their destination");
        return ZZ_E_NOSPACE;
    }
    return ZZ_OK;
}

// ---- a file of gzip members back to back (zz_inflate_members.h) -----------------------------------------------------------
// k_inflate_members over src[0, n) onto dst[0, cap), waited for
static int members_serial_run(zz_ctx* c, const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, hipStream_t st)      // (the result: mem.h_sres)
{
    auto& M = c->dec.mem;
    if (int rc = M.sres.grow(1)) return rc;
    if (int rc = M.h_sres.grow(1)) return rc;
    hipLaunchKernelGGL(k_inflate_members, dim3(1), dim3(ZZ_INF_THREADS), 0, st, src, n, dst, cap, (zz_inf_members_out*)M.sres);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(M.h_sres, M.sres, sizeof(zz_inf_members_out), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}
// the serial path: zi_members by one wavefront; it decides every verdict the blocked path does not. `members0` proven members
// and `out0` bytes of theirs stand in front of src (0 and 0: the whole file); `path` is what the call reports if this succeeds
// or answers "no space"
static int dec_members_serial(zz_ctx* c, const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, hipStream_t st, uint64_t* out_len,
                              uint64_t members0, uint64_t out0, int path)
{
    auto& M = c->dec.mem;
    if (int rc = members_serial_run(c, src, n, dst, cap, st)) return rc;
    M.members = members0 + M.h_sres->members;
    M.path = path;
    if (M.h_sres->status == ZI_ITEM_OK) { *out_len = out0 + M.h_sres->out; return ZZ_OK; }
    if (M.h_sres->status == ZI_ITEM_NOSPACE) {
        set_err("member " + std::to_string(M.members) + " does not fit what is left of the destination");
        return ZZ_E_NOSPACE;
    }
    M.path = 3;
    set_err("what stands where member " + std::to_string(M.members) + " would begin is not a valid gzip member");
    return ZZ_E_DATA;
}

// The front of the blocked path, for zz_decode_members_device and zz_members_index_device: mark (count per stretch, scan, and
// the one number that sizes the candidates' buffers: one readback), fill, check and hop (only if the check failed), enqueued
// and not waited for. *ncand: the candidates; *listed: the member list is being made in mem.offs / mem.lens and mem.st will say
// whether it stands (false: no candidates, or more than one launch's grid holds).
static int members_front(zz_ctx* c, const uint8_t* src, uint64_t src_len, hipStream_t st, uint64_t* ncand_out, bool* listed)
{
    auto& M = c->dec.mem;
    *ncand_out = 0; *listed = false;
    const uint64_t nblk = (src_len + ZZ_MEM_STRETCH - 1) / ZZ_MEM_STRETCH;
    if (nblk > 0x7FFFFFFFull) return ZZ_OK;                              // (8 TiB of source: beyond one launch's grid)
    if (int rc = M.blk_cnt.grow(nblk)) return rc;
    if (int rc = M.blk_base.grow(nblk)) return rc;
    if (int rc = M.st.grow(1)) return rc;
    if (int rc = M.h_st.grow(1)) return rc;
    HIPCHK(hipMemsetAsync(M.st, 0, sizeof(zz_mem_state), st));
    HIPCHK(hipMemsetAsync(&M.st->mstar, 0xFF, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_members_mark<false>, dim3((uint32_t)nblk), dim3(ZZ_MEM_THREADS), 0, st, src, src_len, (uint32_t*)M.blk_cnt,
                       (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_members_scan, dim3(1), dim3(ZZ_MEM_SCAN_THREADS), 0, st, (const uint32_t*)M.blk_cnt, nblk, (uint64_t*)M.blk_base,
                       (zz_mem_state*)M.st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(M.h_st, M.st, sizeof(zz_mem_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t ncand = M.h_st->candidates;
    *ncand_out = ncand;
    if (ncand == 0 || ncand > 0x7FFFFFFFull) return ZZ_OK;
    if (int rc = M.offs.grow(ncand)) return rc;
    if (int rc = M.lens.grow(ncand)) return rc;
    hipLaunchKernelGGL(k_members_mark<true>, dim3((uint32_t)nblk), dim3(ZZ_MEM_THREADS), 0, st, src, src_len, (uint32_t*)M.blk_cnt,
                       (const uint64_t*)M.blk_base, (uint64_t*)M.offs, (uint32_t*)M.lens);
    HIPCHK(hipGetLastError());
    const uint64_t cgrid = (ncand + 255) / 256;
    hipLaunchKernelGGL(k_members_check, dim3((uint32_t)(cgrid < 2048 ? cgrid : 2048)), dim3(256), 0, st, (const uint64_t*)M.offs,
                       (const uint32_t*)M.lens, ncand, src_len, (zz_mem_state*)M.st);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_members_hop, dim3(1), dim3(ZZ_WAVE), 0, st, src, src_len, (uint64_t*)M.offs, (uint32_t*)M.lens, ncand,
                       (zz_mem_state*)M.st);
    HIPCHK(hipGetLastError());
    *listed = true;
    return ZZ_OK;
}

extern "C" int zz_decode_members_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, void* d_dst_v, uint64_t cap, uint64_t* out_len,
                                        void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (!out_len) { set_err("null out_len"); return ZZ_E_ARG; }
    if (!d_src_v && src_len) { set_err("null source"); return ZZ_E_ARG; }
    if (!d_dst_v && cap) { set_err("null destination"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    auto& M = c->dec.mem;
    M.members = 0; M.candidates = 0; M.path = 0;
    if (src_len == 0) { set_err("an empty file holds no gzip member"); return ZZ_E_DATA; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint8_t* src = (const uint8_t*)d_src_v;
    uint8_t* dst = (uint8_t*)d_dst_v;
    const auto serial = [&]() -> int { return dec_members_serial(c, src, src_len, dst, cap, st, out_len, 0, 0, 3); };     // (writes *out_len on ZZ_OK only)

    uint64_t ncand = 0; bool listed = false;
    if (int rc = members_front(c, src, src_len, st, &ncand, &listed)) return rc;
    M.candidates = ncand;
    if (!listed) return serial();

    // slots: one readback for fill, check, hop (only if the check failed) and slots
    if (int rc = ensure_member_items(c, ncand)) return rc;
    zz_mem_slots q;
    q.src = src; q.n = src_len; q.dst = dst; q.cap = cap; q.offs = M.offs; q.lens = M.lens;
    q.srcs = M.srcs; q.src_lens = M.src_lens; q.dsts = M.dsts; q.caps = M.caps; q.st = M.st;
    hipLaunchKernelGGL(k_members_slots, dim3(1), dim3(ZZ_MEM_SCAN_THREADS), 0, st, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(M.h_st, M.st, sizeof(zz_mem_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!M.h_st->blocked) return serial();
    const uint64_t members = M.h_st->members, mstar = M.h_st->mstar;
    const bool have_mstar = mstar != ~0ull;
    const uint64_t dealt = have_mstar ? mstar + 1 : members;

    // decode: k_inflate_items over the dealt members, as zz_decode_batch_device launches it
    if (int rc = dec_items(c, member_items_params(c, (uint32_t)dealt, nullptr), st)) return rc;
    const int v = zi_members_verdict(have_mstar, c->dec.items_host[0], c->dec.items_host[1]);
    if (v == ZI_MEMBERS_SERIAL) return serial();
    const int path = M.h_st->chain_bad ? 2 : 1;
    if (v == ZI_MEMBERS_REJUDGE) {
        // m* alone failed, for want of room -- on its cut-out bytes, which proves nothing about the bits behind them: the serial
        // rule from m* on gives the verdict (for an honest file: one member's work, and the same answer)
        const uint64_t at = M.h_st->mstar_src, off = M.h_st->mstar_dst;
        return dec_members_serial(c, src + at, src_len - at, dst + off, cap - off, st, out_len, mstar, off, path);
    }
    M.path = path; M.members = dealt;
    *out_len = M.h_st->total;
    return ZZ_OK;
}
extern "C" int zz_ctx_last_decode_members_stats(const zz_ctx* c, uint64_t* members, uint64_t* candidates, int* path)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (members) *members = c->dec.mem.members;
    if (candidates) *candidates = c->dec.mem.candidates;
    if (path) *path = c->dec.mem.path;
    return ZZ_OK;
}

// ---- a blocked file's index, and reads through it (zz_inflate_members_ranges.h) -----------------------------------------------
extern "C" int zz_members_index_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, uint64_t* d_index, uint64_t max_entries,
                                       uint64_t* entries, void* hip_stream)
{
    if (entries) *entries = 0;
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (!entries) { set_err("null entries"); return ZZ_E_ARG; }
    if (!d_src_v && src_len) { set_err("null source"); return ZZ_E_ARG; }
    if (!d_index && max_entries) { set_err("null index"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    if (src_len == 0) { set_err("an empty file holds no gzip member"); return ZZ_E_DATA; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint8_t* src = (const uint8_t*)d_src_v;
    auto& M = c->dec.mem;
    uint64_t ncand = 0; bool listed = false;
    if (int rc = members_front(c, src, src_len, st, &ncand, &listed)) return rc;
    if (listed) {
        HIPCHK(hipMemcpyAsync(M.h_st, M.st, sizeof(zz_mem_state), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (!listed || !M.h_st->blocked) {
        set_err("not a blocked file: its members do not announce their lengths (BC) one after the other; zz_decode_members_device decodes it");
        return ZZ_E_UNSUPPORTED;
    }
    const uint64_t members = M.h_st->members;
    *entries = members + 1;
    if (max_entries < members + 1) { set_err("the index has " + std::to_string(members + 1) + " entries"); return ZZ_E_NOSPACE; }
    hipLaunchKernelGGL(k_members_pairs, dim3(1), dim3(ZZ_MR_SCAN_THREADS), 0, st, src, src_len, (const uint64_t*)M.offs, (const uint32_t*)M.lens,
                       members, d_index);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

// ---- the members of any member file, found (zz_inflate_members_find.h; the rules in zz_inflate_core.h) ---------------------------
// one round of measures: one launch, the records back (all of them: a round's jobs write into the candidates' own records)
static int mf_run_round(zz_ctx* c, const uint8_t* src, uint64_t n, uint64_t ncand, const uint32_t* h_which, uint64_t njobs, uint64_t limit,
                        std::vector<zi_find_job>& rec, hipStream_t st)
{
    auto& F = c->dec.mf;
    if (h_which) HIPCHK(hipMemcpyAsync(F.which, h_which, njobs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(F.next, 0, sizeof(unsigned int), st));
    zz_mf_params Q = {};
    Q.src = src; Q.n = n; Q.offs = c->dec.mem.offs; Q.rec = F.rec; Q.which = h_which ? (const uint32_t*)F.which : nullptr;
    Q.njobs = (uint32_t)njobs; Q.limit = limit; Q.next = F.next;
    const uint64_t resident = 256ull * ZZ_MF_WG_PER_CU;
    hipLaunchKernelGGL(k_members_reach, dim3((uint32_t)(njobs < resident ? njobs : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rec.data(), F.rec, ncand * sizeof(zi_find_job), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ++F.rounds;
    return ZZ_OK;
}
// The front of both calls: mark (count per stretch, scan, one readback that sizes everything by the candidates), fill, the
// measures of round 1, the walk, round 2 where the walk met a job that gave up, the walk again. *walk: ZI_MF_CLEAN or
// ZI_MF_BROKEN, or -1: more than one launch's grid holds (stretches or candidates above 2^31 - 1). Behind a clean walk rec (on
// the host and in mf.rec) and keep (on the host) describe the members, and the call's stats are set.
static int mf_front(zz_ctx* c, const uint8_t* src, uint64_t src_len, uint64_t limit_bytes, hipStream_t st, std::vector<zi_find_job>& rec,
                    std::vector<uint8_t>& keep, int* walk)
{
    auto& M = c->dec.mem;
    auto& F = c->dec.mf;
    *walk = -1;
    const uint64_t nblk = (src_len + ZZ_MEM_STRETCH - 1) / ZZ_MEM_STRETCH;
    if (nblk > 0x7FFFFFFFull) return ZZ_OK;                              // (8 TiB of source)
    if (int rc = M.blk_cnt.grow(nblk)) return rc;
    if (int rc = M.blk_base.grow(nblk)) return rc;
    if (int rc = M.st.grow(1)) return rc;
    if (int rc = M.h_st.grow(1)) return rc;
    HIPCHK(hipMemsetAsync(M.st, 0, sizeof(zz_mem_state), st));
    hipLaunchKernelGGL(k_members_find_mark<false>, dim3((uint32_t)nblk), dim3(ZZ_MEM_THREADS), 0, st, src, src_len, (uint32_t*)M.blk_cnt,
                       (const uint64_t*)nullptr, (uint64_t*)nullptr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_members_scan, dim3(1), dim3(ZZ_MEM_SCAN_THREADS), 0, st, (const uint32_t*)M.blk_cnt, nblk, (uint64_t*)M.blk_base,
                       (zz_mem_state*)M.st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(M.h_st, M.st, sizeof(zz_mem_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t ncand = M.h_st->candidates;                            // (at least one: offset 0)
    F.candidates = ncand;
    if (ncand == 0 || ncand > 0x7FFFFFFFull) return ZZ_OK;
    if (int rc = M.offs.grow(ncand)) return rc;
    if (int rc = F.rec.grow(ncand)) return rc;
    if (int rc = F.keep.grow(ncand)) return rc;
    if (int rc = F.which.grow(ncand)) return rc;
    if (int rc = F.next.grow(1)) return rc;
    hipLaunchKernelGGL(k_members_find_mark<true>, dim3((uint32_t)nblk), dim3(ZZ_MEM_THREADS), 0, st, src, src_len, (uint32_t*)M.blk_cnt,
                       (const uint64_t*)M.blk_base, (uint64_t*)M.offs);
    HIPCHK(hipGetLastError());
    rec.resize(ncand); keep.assign(ncand, 0);
    if (int rc = mf_run_round(c, src, src_len, ncand, nullptr, ncand, limit_bytes, rec, st)) return rc;
    zi_mf_walk W{ 0, 0, 0, 0 };
    const zi_view<const zi_find_job> recs{ rec.data(), ncand };
    int v = zi_mf_link(W, recs, ncand, src_len, zi_view<uint8_t>{ keep.data(), ncand });
    if (v == ZI_MF_MORE) {
        std::vector<uint32_t> which(zi_mf_again(W, recs, ncand, nullptr));
        zi_mf_again(W, recs, ncand, which.data());
        if (int rc = mf_run_round(c, src, src_len, ncand, which.data(), which.size(), ZI_FIND_NONE, rec, st)) return rc;
        v = zi_mf_link(W, recs, ncand, src_len, zi_view<uint8_t>{ keep.data(), ncand });
        if (v == ZI_MF_MORE) v = ZI_MF_BROKEN;                            // (a job without a limit does not give up)
    }
    F.members = W.members; F.dropped = W.dropped;
    *walk = v;
    return ZZ_OK;
}
// the slots behind a clean walk: the flags up, one launch, mf.h_st back. The descriptors go to mem's arrays when `dst_side` is set,
// the index rows to d_index when it is not null
static int mf_slots(zz_ctx* c, const uint8_t* src, uint64_t src_len, uint8_t* dst, uint64_t cap, bool dst_side, uint64_t* d_index,
                    const std::vector<uint8_t>& keep, hipStream_t st)
{
    auto& M = c->dec.mem;
    auto& F = c->dec.mf;
    if (int rc = F.st.grow(1)) return rc;
    if (int rc = F.h_st.grow(1)) return rc;
    HIPCHK(hipMemcpyAsync(F.keep, keep.data(), keep.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(F.st, 0, sizeof(zz_mf_state), st));
    HIPCHK(hipMemsetAsync(&F.st->mstar, 0xFF, sizeof(unsigned long long), st));
    zz_mf_slots q = {};
    q.src = src; q.n = src_len; q.dst = dst; q.cap = cap; q.rec = F.rec; q.keep = F.keep; q.nc = keep.size();
    if (dst_side) { q.srcs = M.srcs; q.src_lens = M.src_lens; q.dsts = M.dsts; q.caps = M.caps; }
    q.idx = d_index; q.st = F.st;
    hipLaunchKernelGGL(k_members_find_slots, dim3(1), dim3(ZZ_MEM_SCAN_THREADS), 0, st, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(F.h_st, F.st, sizeof(zz_mf_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

extern "C" int zz_members_find_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, uint64_t limit_bytes, uint64_t* d_index,
                                      uint64_t max_entries, uint64_t* entries, void* hip_stream)
{
    if (entries) *entries = 0;
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (!entries) { set_err("null entries"); return ZZ_E_ARG; }
    if (!d_src_v && src_len) { set_err("null source"); return ZZ_E_ARG; }
    if (!d_index && max_entries) { set_err("null index"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    auto& F = c->dec.mf;
    F.members = 0; F.candidates = 0; F.dropped = 0; F.rounds = 0;
    if (src_len == 0) { set_err("an empty file holds no gzip member"); return ZZ_E_DATA; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint8_t* src = (const uint8_t*)d_src_v;
    std::vector<zi_find_job> rec; std::vector<uint8_t> keep;
    int walk = -1;
    if (int rc = mf_front(c, src, src_len, limit_bytes ? limit_bytes : ZZ_MEMBERS_FIND_LIMIT_DEFAULT, st, rec, keep, &walk)) return rc;
    if (walk < 0) { set_err("more than 2^31 - 1 places where a gzip header stands: zz_decode_members_device decodes such a file"); return ZZ_E_UNSUPPORTED; }
    if (walk != ZI_MF_CLEAN) {
        set_err("not a file of gzip members: the chain from offset 0 breaks behind member " + std::to_string(F.members));
        return ZZ_E_DATA;
    }
    *entries = F.members + 1;
    if (max_entries < F.members + 1) { set_err("the index has " + std::to_string(F.members + 1) + " entries"); return ZZ_E_NOSPACE; }
    return mf_slots(c, src, src_len, nullptr, 0, false, d_index, keep, st);
}

extern "C" int zz_decode_members_found_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, void* d_dst_v, uint64_t cap, uint64_t* out_len,
                                              void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (!out_len) { set_err("null out_len"); return ZZ_E_ARG; }
    if (!d_src_v && src_len) { set_err("null source"); return ZZ_E_ARG; }
    if (!d_dst_v && cap) { set_err("null destination"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    auto& M = c->dec.mem;
    auto& F = c->dec.mf;
    F.members = 0; F.candidates = 0; F.dropped = 0; F.rounds = 0;
    if (src_len == 0) { set_err("an empty file holds no gzip member"); return ZZ_E_DATA; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint8_t* src = (const uint8_t*)d_src_v;
    uint8_t* dst = (uint8_t*)d_dst_v;
    // zi_members over what is left behind `members0` proven members (`at` source bytes, `off` decoded bytes): its answer is the call's
    const auto serial = [&](uint64_t members0, uint64_t at, uint64_t off) -> int {
        if (int rc = members_serial_run(c, src + at, src_len - at, dst + off, cap - off, st)) return rc;
        const zz_inf_members_out& R = *M.h_sres;
        const uint64_t member = members0 + R.members;
        if (R.status == ZI_ITEM_OK) { *out_len = off + R.out; return ZZ_OK; }
        if (R.status == ZI_ITEM_NOSPACE) { set_err("member " + std::to_string(member) + " does not fit what is left of the destination"); return ZZ_E_NOSPACE; }
        set_err("what stands where member " + std::to_string(member) + " would begin is not a valid gzip member");
        return ZZ_E_DATA;
    };

    std::vector<zi_find_job> rec; std::vector<uint8_t> keep;
    int walk = -1;
    if (int rc = mf_front(c, src, src_len, ZZ_MEMBERS_FIND_LIMIT_DEFAULT, st, rec, keep, &walk)) return rc;
    if (walk != ZI_MF_CLEAN) return serial(0, 0, 0);                     // a broken walk, or too many candidates: the whole file
    if (int rc = ensure_member_items(c, F.members)) return rc;
    if (int rc = F.status.grow(F.members)) return rc;
    if (int rc = mf_slots(c, src, src_len, dst, cap, true, nullptr, keep, st)) return rc;
    const uint64_t members = F.h_st->members, mstar = F.h_st->mstar;
    const bool have_mstar = mstar != ~0ull;
    const uint64_t dealt = have_mstar ? mstar : members;

    // decode: k_inflate_items over the members in front of m*, as zz_decode_batch_device launches it
    unsigned long long failed = 0;
    if (dealt) {
        if (int rc = dec_items(c, member_items_params(c, (uint32_t)dealt, F.status), st)) return rc;
        failed = c->dec.items_host[0] + c->dec.items_host[1];
    }
    if (!failed && !have_mstar) { *out_len = F.h_st->total; return ZZ_OK; }
    // the first member that did not answer ZZ_OK, or m*: the members in front of it are proven, zi_members decides from there on
    uint64_t first = dealt, at = F.h_st->mstar_src, off = F.h_st->mstar_dst;
    if (failed) {
        std::vector<int32_t> status(dealt);
        HIPCHK(hipMemcpyAsync(status.data(), F.status, dealt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        uint64_t j = 0, sum = 0;
        for (uint64_t k = 0; k < keep.size(); ++k) {
            if (!keep[k]) continue;
            if (j >= dealt) break;
            if (status[j] != ZI_ITEM_OK) { first = j; at = rec[k].a; off = sum; break; }
            sum += rec[k].c; ++j;
        }
    }
    return serial(first, at, off);
}

extern "C" int zz_ctx_last_members_find_stats(const zz_ctx* c, uint64_t* members, uint64_t* candidates, uint64_t* dropped, uint32_t* rounds)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (members) *members = c->dec.mf.members;
    if (candidates) *candidates = c->dec.mf.candidates;
    if (dropped) *dropped = c->dec.mf.dropped;
    if (rounds) *rounds = c->dec.mf.rounds;
    return ZZ_OK;
}

// ---- points inside members: one index over members and blocks (zz_inflate_members_points.h; the rules in
// zz_inflate_core.h) ---------------------------------------------------------------------------------------------------------------
// one round's jobs: up, one launch, the results back in place (want[0, njobs))
static int mp_run_jobs(zz_ctx* c, const uint8_t* src, uint64_t n, uint64_t nb, uint64_t chunk, zi_mp_job* want, uint64_t njobs, hipStream_t st)
{
    auto& P = c->dec.mp;
    HIPCHK(hipMemcpyAsync(P.job, want, njobs * sizeof(zi_mp_job), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(P.next, 0, sizeof(unsigned int), st));
    zz_mp_params Q = {};
    Q.src = src; Q.n = n; Q.bc = P.bc; Q.nb = nb; Q.chunk = chunk; Q.job = P.job; Q.njobs = (uint32_t)njobs; Q.next = P.next;
    const uint64_t resident = 256ull * ZZ_MP_WG_PER_CU;
    hipLaunchKernelGGL(k_members_points_reach, dim3((uint32_t)(njobs < resident ? njobs : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(want, P.job, njobs * sizeof(zi_mp_job), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZZ_OK;
}

extern "C" int zz_members_points_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, uint64_t chunk_bytes, uint64_t spacing,
                                        uint64_t* points, uint64_t max_entries, uint64_t* entries, uint64_t* out_len, void* hip_stream)
{
    if (entries) *entries = 0;
    if (out_len) *out_len = 0;
    if (!c || !entries || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    if (!d_src_v && src_len) { set_err("null source"); return ZZ_E_ARG; }
    if (!points && max_entries) { set_err("null index"); return ZZ_E_ARG; }
    if (chunk_bytes < 16) { set_err("chunk_bytes must be at least 16"); return ZZ_E_ARG; }
    if (spacing == 0) { set_err("spacing must be at least 1"); return ZZ_E_ARG; }
    if (src_len > (~0ull >> 3)) { set_err("src_len must be below 2^61"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    auto& M = c->dec.mem;
    auto& F = c->dec.pf;
    auto& P = c->dec.mp;
    P.members_found = 0; P.header_candidates = 0; P.block_candidates = 0; P.dropped = 0; P.rounds = 0;
    if (src_len == 0) { set_err("an empty file holds no gzip member"); return ZZ_E_DATA; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint8_t* src = (const uint8_t*)d_src_v;
    const char* too_many = "more than 2^31 - 1 candidates: zz_decode_members_device decodes such a file";
    // the header candidates: zz_members_find_device's mark passes
    const uint64_t nblk = (src_len + ZZ_MEM_STRETCH - 1) / ZZ_MEM_STRETCH;
    const uint64_t chunks = zi_find_chunks(src_len, chunk_bytes);
    if (nblk > 0x7FFFFFFFull || chunks > 0x7FFFFFFFull) { set_err(too_many); return ZZ_E_UNSUPPORTED; }
    if (int rc = M.blk_cnt.grow(nblk)) return rc;
    if (int rc = M.blk_base.grow(nblk)) return rc;
    if (int rc = M.st.grow(1)) return rc;
    if (int rc = M.h_st.grow(1)) return rc;
    if (int rc = P.next.grow(1)) return rc;
    HIPCHK(hipMemsetAsync(M.st, 0, sizeof(zz_mem_state), st));
    hipLaunchKernelGGL(k_members_find_mark<false>, dim3((uint32_t)nblk), dim3(ZZ_MEM_THREADS), 0, st, src, src_len, (uint32_t*)M.blk_cnt,
                       (const uint64_t*)nullptr, (uint64_t*)nullptr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_members_scan, dim3(1), dim3(ZZ_MEM_SCAN_THREADS), 0, st, (const uint32_t*)M.blk_cnt, nblk, (uint64_t*)M.blk_base,
                       (zz_mem_state*)M.st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(M.h_st, M.st, sizeof(zz_mem_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t nh = M.h_st->candidates;                                // (at least one: offset 0)
    P.header_candidates = nh;
    if (nh == 0 || nh > 0x7FFFFFFFull) { set_err(too_many); return ZZ_E_UNSUPPORTED; }
    if (int rc = M.offs.grow(nh)) return rc;
    hipLaunchKernelGGL(k_members_find_mark<true>, dim3((uint32_t)nblk), dim3(ZZ_MEM_THREADS), 0, st, src, src_len, (uint32_t*)M.blk_cnt,
                       (const uint64_t*)M.blk_base, (uint64_t*)M.offs);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> hc(nh), bc;
    HIPCHK(hipMemcpyAsync(hc.data(), M.offs, nh * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    // the block candidates: zz_points_index_device's finder with D = the file
    const uint64_t resident = 256ull * ZZ_PF_WG_PER_CU;
    if (chunks > 1) {
        if (int rc = F.job.grow(chunks + 2)) return rc;
        if (int rc = F.next.grow(1)) return rc;
        std::vector<zi_find_job> rec(chunks);
        HIPCHK(hipMemsetAsync(F.next, 0, sizeof(unsigned int), st));
        zz_pf_params Q = {};
        Q.d = src; Q.n = src_len; Q.chunk = chunk_bytes; Q.chunks = chunks; Q.job = F.job; Q.next = F.next;
        hipLaunchKernelGGL(k_points_find, dim3((uint32_t)(chunks - 1 < resident ? chunks - 1 : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rec.data(), F.job, chunks * sizeof(zi_find_job), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint64_t k = 1; k < chunks; ++k) if (rec[k].a != ZI_FIND_NONE) bc.push_back(rec[k].a);
    }
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t nb = bc.size();
    P.block_candidates = nb;
    if (int rc = P.bc.grow(nb + 1)) return rc;
    if (int rc = P.job.grow(nh + nb + 2)) return rc;
    if (nb) HIPCHK(hipMemcpyAsync(P.bc, bc.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // the jobs, the walk and its repair rounds
    std::vector<zi_mp_job> rh(nh + 1), rb(nb + 1), rr(nb + 1), want(nh + nb + 2);
    std::vector<uint64_t> acc(2 * (2 * nh + nb) + 2);
    memset(rh.data(), 0, rh.size() * sizeof(zi_mp_job)); memset(rb.data(), 0, rb.size() * sizeof(zi_mp_job));
    memset(rr.data(), 0, rr.size() * sizeof(zi_mp_job));
    zi_mp_walk W{ zi_view<const uint64_t>{ hc.data(), nh }, nh, zi_view<const uint64_t>{ bc.data(), nb }, nb, zi_view<zi_mp_job>{ rh.data(), nh },
                  zi_view<zi_mp_job>{ rb.data(), nb }, zi_view<zi_mp_job>{ rr.data(), nb + 1 }, zi_view<uint64_t>{ acc.data(), 2 * (2 * nh + nb) }, 0,
                  src_len, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    uint64_t nwant = nh + nb;
    for (uint64_t i = 0; i < nwant; ++i) want[i] = zi_mp_first_job(W, i);
    int verdict;
    for (;;) {
        ++P.rounds;
        if (int rc = mp_run_jobs(c, src, src_len, nb, chunk_bytes, want.data(), nwant, st)) return rc;
        for (uint64_t j = 0; j < nwant; ++j) zi_mp_store(W, want[j]);
        verdict = zi_mp_link(W, zi_view<zi_mp_job>{ want.data(), want.size() }, &nwant);
        if (verdict != ZI_FW_MORE) break;
        if (P.rounds > 3 * (nh + nb) + 2) { set_err("the walk over members and blocks did not close"); return ZZ_E_DATA; }   // (every round confirms a job)
    }
    P.members_found = W.members; P.dropped = zi_mp_dropped(W);
    if (verdict == ZI_FW_DATA) {
        set_err("not a file of gzip members: the walk from offset 0 breaks behind member " + std::to_string(W.members));
        return ZZ_E_DATA;
    }
    *entries = zi_mp_rows(W, spacing, nullptr, 0);
    *out_len = W.bytes;
    if (max_entries < *entries) { set_err("the index has " + std::to_string(*entries) + " entries"); return ZZ_E_NOSPACE; }
    zi_mp_rows(W, spacing, points, max_entries);
    return ZZ_OK;
}

extern "C" int zz_ctx_last_members_points_stats(const zz_ctx* c, uint64_t* members, uint64_t* header_candidates, uint64_t* block_candidates,
                                                uint64_t* dropped, uint32_t* rounds)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (members) *members = c->dec.mp.members_found;
    if (header_candidates) *header_candidates = c->dec.mp.header_candidates;
    if (block_candidates) *block_candidates = c->dec.mp.block_candidates;
    if (dropped) *dropped = c->dec.mp.dropped;
    if (rounds) *rounds = c->dec.mp.rounds;
    return ZZ_OK;
}

extern "C" int zz_members_points_to_index(const uint64_t* points, uint64_t entries, uint64_t* index, uint64_t max_entries, uint64_t* index_entries)
{
    if (index_entries) *index_entries = 0;
    if (!points || !index_entries || (!index && max_entries)) { set_err("null argument"); return ZZ_E_ARG; }
    const uint64_t n = zi_mp_to_index(points, entries, nullptr, 0);
    if (n == 0) { set_err("the rows are no member point index: START, inner rows and END per member"); return ZZ_E_DATA; }
    *index_entries = n;
    if (max_entries < n) { set_err("the index has " + std::to_string(n) + " entries"); return ZZ_E_NOSPACE; }
    zi_mp_to_index(points, entries, index, max_entries);
    return ZZ_OK;
}

// ---- decode through a member point index (zz_inflate_members_decode.h; the rules, zi_mpd_*, in zz_inflate_core.h) ---------------
// One batch: descriptors [k0, k0 + nseg) of the call through phase 1, the tile counts, the rounds and the sums. *failed: segments
// whose run was refused (the rounds and the sums still run: pointers never leave their member, so the members that hold no refused
// segment end up whole). The host waits once, and once more behind the rounds if anything is pending.
static int mpd_batch(zz_ctx* c, const uint8_t* src, uint64_t n, const zi_mpd_seg* seg, uint64_t k0, uint32_t nseg, uint8_t* dst,
                     hipStream_t st, unsigned long long* failed)
{
    auto& D = c->dec;
    auto& X = D.mpd;
    const uint32_t words = ZI_POINTS_TILE / 32;
    const uint64_t resident = 256ull * ZZ_MPD_WG_PER_CU;
    const uint64_t base = seg[k0].o0, nbytes = seg[k0 + nseg - 1].o1 - base;
    const uint32_t tiles = (uint32_t)((nbytes + ZI_POINTS_TILE - 1) / ZI_POINTS_TILE);
    const uint32_t grid = (uint32_t)(nseg < resident ? nseg : resident);
    HIPCHK(hipMemsetAsync(D.tot, 0, ZZ_TOT_SLOTS * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(X.next, 0, sizeof(unsigned int), st));
    if (tiles) HIPCHK(hipMemsetAsync(D.pend, 0, (uint64_t)tiles * words * 4, st));
    zz_mpd_params Q;
    Q.src = src; Q.n = n; Q.seg = X.seg; Q.k0 = k0; Q.nseg = nseg; Q.dst = dst; Q.base = base; Q.nbytes = nbytes;
    Q.st = D.st; Q.pend = D.pend; Q.words = (uint64_t)tiles * words; Q.segok = X.segok; Q.sums = X.sums; Q.next = X.next; Q.tot = D.tot;
    hipLaunchKernelGGL(k_members_segments, dim3(grid), dim3(ZZ_INF_THREADS), 0, st, Q);
    if (tiles) hipLaunchKernelGGL(k_points_count, dim3(tiles), dim3(256), 0, st, D.pend, D.pcnt, D.prem, D.tot);
    HIPCHK(hipGetLastError());
    unsigned long long tot[ZZ_TOT_SLOTS];
    if (int rc = dec_read_tot(c, tot, st)) return rc;
    *failed = tot[ZZ_TOT_FAILED];
    ++X.batches;
    if (tot[ZZ_TOT_PENDING] != 0) {
        const uint32_t rounds = zz_inf_rounds(nseg);                        // a chain has at most one link per segment of a batch
        zz_res_params R{ dst, base, ZI_POINTS_TILE, tiles, words, D.st, D.pend, D.pcnt, D.prem, D.tot };
        for (uint32_t r = 1; r <= rounds; ++r) hipLaunchKernelGGL(k_inflate_resolve, dim3(tiles), dim3(ZZ_INF_RES_THREADS), 0, st, R, r);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(X.next, 0, sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_members_sums, dim3(grid), dim3(ZZ_INF_THREADS), 0, st, Q);
    HIPCHK(hipGetLastError());
    if (tot[ZZ_TOT_PENDING] != 0) {
        const uint32_t rounds = zz_inf_rounds(nseg);
        const unsigned long long pending = tot[ZZ_TOT_PENDING];
        if (int rc = dec_read_tot(c, tot, st)) return rc;
        if (tot[ZZ_TOT_OPEN + rounds] != 0) *failed += 1;                   // (cannot happen: the rounds suffice for any chain)
        uint32_t r = 1;
        while (r < rounds && tot[ZZ_TOT_OPEN + r] != 0) ++r;
        X.pending += pending;
        X.rounds = std::max(X.rounds, r);
    }
    return ZZ_OK;
}

extern "C" int zz_decode_members_points_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, void* d_dst_v, uint64_t cap, uint64_t* out_len,
                                               const uint64_t* points, uint64_t entries, uint64_t batch_bytes, void* hip_stream)
{
    if (out_len) *out_len = ~0ull;
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    {   // the stats say "refused before anything ran" from here on
        auto& X0 = c->dec.mpd;
        X0.members = 0; X0.proven = 0; X0.segments = 0; X0.pending = 0; X0.batches = 0; X0.rounds = 0; X0.serial = 0;
    }
    if (!out_len) { set_err("null out_len"); return ZZ_E_ARG; }
    if (!d_src_v && src_len) { set_err("null source"); return ZZ_E_ARG; }
    if (!d_dst_v && cap) { set_err("null destination"); return ZZ_E_ARG; }
    if (!points && entries) { set_err("null points with entries > 0 (the rows live in host memory; NULL and 0: the call makes them)"); return ZZ_E_ARG; }
    if (entries == 1) { set_err("a member point index has at least two rows"); return ZZ_E_ARG; }
    if (batch_bytes > ZZ_INF_BATCH_BYTES) { set_err("batch_bytes must be at most 64 MiB (0: 64 MiB)"); return ZZ_E_ARG; }
    if (call_pending(c)) return ZZ_E_ARG;
    auto& D = c->dec;
    auto& M = D.mem;
    auto& X = D.mpd;
    if (src_len == 0) { set_err("an empty file holds no gzip member"); return ZZ_E_DATA; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint8_t* src = (const uint8_t*)d_src_v;
    uint8_t* dst = (uint8_t*)d_dst_v;
    const uint64_t limit = batch_bytes ? batch_bytes : ZZ_INF_BATCH_BYTES;
    // zi_members over what is left behind `members0` proven members (`at` source bytes, `off` decoded bytes): its answer is the call's
    const auto serial = [&](uint64_t members0, uint64_t at, uint64_t off) -> int {
        X.serial = 1; X.proven = members0;
        if (int rc = members_serial_run(c, src + at, src_len - at, dst + off, cap - off, st)) return rc;
        const zz_inf_members_out& R = *M.h_sres;
        const uint64_t member = members0 + R.members;
        if (R.status == ZI_ITEM_OK) { *out_len = off + R.out; return ZZ_OK; }
        if (R.status == ZI_ITEM_NOSPACE) { set_err("member " + std::to_string(member) + " does not fit what is left of the destination"); return ZZ_E_NOSPACE; }
        set_err("what stands where member " + std::to_string(member) + " would begin is not a valid gzip member");
        return ZZ_E_DATA;
    };

    // the rows: the caller's, or the call's own (its index call's stats are put back: this call leaves the other calls' alone)
    std::vector<uint64_t> own;
    if (!points) {
        const auto keep = std::make_tuple(D.mp.members_found, D.mp.header_candidates, D.mp.block_candidates, D.mp.dropped, D.mp.rounds);
        uint64_t need = 0, total = 0;
        int rc = zz_members_points_device(c, d_src_v, src_len, ZZ_POINTS_CHUNK_DEFAULT, 1, nullptr, 0, &need, &total, hip_stream);
        if (rc == ZZ_E_NOSPACE) {
            own.resize(2 * need);
            rc = zz_members_points_device(c, d_src_v, src_len, ZZ_POINTS_CHUNK_DEFAULT, 1, own.data(), need, &need, &total, hip_stream);
        }
        std::tie(D.mp.members_found, D.mp.header_candidates, D.mp.block_candidates, D.mp.dropped, D.mp.rounds) = keep;
        if (rc == ZZ_E_HIP) return rc;
        if (rc != ZZ_OK) return serial(0, 0, 0);
        points = own.data(); entries = need;
    }
    // the check, the members and the descriptors
    uint64_t nmem = 0, nseg = 0;
    if (!zi_mpd_plan(points, entries, src_len, nullptr, 0, nullptr, 0, &nmem, &nseg)) return serial(0, 0, 0);
    std::vector<zi_mpd_member> mem(nmem);
    std::vector<zi_mpd_seg> seg(nseg);
    zi_mpd_plan(points, entries, src_len, mem.data(), nmem, seg.data(), nseg, &nmem, &nseg);
    X.members = nmem;
    const uint64_t mstar = zi_mpd_mstar(mem.data(), nmem, cap, limit);
    const uint64_t dealt = mstar, dsegs = mstar < nmem ? mem[mstar].seg0 : nseg;
    X.segments = dsegs;
    if (dealt == 0) return serial(0, 0, 0);
    if (dealt > 0x7FFFFFFFull) return serial(0, 0, 0);                      // (beyond one launch's dealing counter)
    // the workspace: the largest batch, and per descriptor and member of the call
    uint64_t max_bytes = 1, max_segs = 1;
    for (uint64_t k0 = 0, k1; k0 < dsegs; k0 = k1) {
        k1 = zi_mpd_batch(seg.data(), dsegs, k0, limit, ZZ_PT_BATCH_SEGMENTS);
        max_bytes = std::max(max_bytes, seg[k1 - 1].o1 - seg[k0].o0);
        max_segs = std::max(max_segs, k1 - k0);
    }
    const bool have = dec_have(dec_points_workspace(c, max_bytes, max_segs)) && dec_have(D.tot.grow(ZZ_TOT_SLOTS)) &&
                      dec_have(X.seg.grow(dsegs)) && dec_have(X.mem.grow(dealt)) && dec_have(X.segok.grow(dsegs)) && dec_have(X.sums.grow(dsegs)) &&
                      dec_have(X.status.grow(dealt)) && dec_have(X.first_bad.grow(1)) && dec_have(X.next.grow(1));
    if (!have) return serial(0, 0, 0);
    HIPCHK(hipMemcpyAsync(X.seg, seg.data(), dsegs * sizeof(zi_mpd_seg), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(X.mem, mem.data(), dealt * sizeof(zi_mpd_member), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(X.segok, 0, dsegs, st));
    HIPCHK(hipMemsetAsync(X.first_bad, 0xFF, sizeof(unsigned long long), st));
    // the batches; those behind the first that reports a refused segment are not launched (their segments' flags stay 0)
    for (uint64_t k0 = 0, k1; k0 < dsegs; k0 = k1) {
        k1 = zi_mpd_batch(seg.data(), dsegs, k0, limit, ZZ_PT_BATCH_SEGMENTS);
        unsigned long long failed = 0;
        if (int rc = mpd_batch(c, src, src_len, seg.data(), k0, (uint32_t)(k1 - k0), dst, st, &failed)) return rc;
        if (failed) break;
    }
    // the verdict, and the one word the host reads of it
    HIPCHK(hipMemsetAsync(X.next, 0, sizeof(unsigned int), st));
    zz_mpd_verdict_params V;
    V.src = src; V.n = src_len; V.mem = X.mem; V.nmem = (uint32_t)dealt; V.seg = X.seg; V.sums = X.sums; V.segok = X.segok;
    V.status = X.status; V.first_bad = X.first_bad; V.next = X.next;
    const uint64_t resident = 256ull * ZZ_MPD_WG_PER_CU;
    hipLaunchKernelGGL(k_members_verdict, dim3((uint32_t)(dealt < resident ? dealt : resident)), dim3(ZZ_INF_THREADS), 0, st, V);
    HIPCHK(hipGetLastError());
    unsigned long long first_bad = 0;
    HIPCHK(hipMemcpyAsync(&first_bad, X.first_bad, sizeof first_bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t f = first_bad < dealt ? (uint64_t)first_bad : mstar;     // the first dealt member not proven, or m*
    if (f == nmem) { X.proven = nmem; *out_len = mem[nmem - 1].off + mem[nmem - 1].out; return ZZ_OK; }
    return serial(f, mem[f].c, mem[f].off);
}

extern "C" int zz_ctx_last_decode_members_points_stats(const zz_ctx* c, uint64_t* members, uint64_t* proven, uint64_t* segments,
                                                       uint32_t* batches, uint64_t* pending_bytes, uint32_t* rounds, int* serial)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    const auto& X = c->dec.mpd;
    if (members) *members = X.members;
    if (proven) *proven = X.proven;
    if (segments) *segments = X.segments;
    if (batches) *batches = X.batches;
    if (pending_bytes) *pending_bytes = X.pending;
    if (rounds) *rounds = X.rounds;
    if (serial) *serial = X.serial;
    return ZZ_OK;
}

// ---- reads through an index: the one procedure of zz_decode_members_ranges_device and zz_decode_points_ranges_device ------------
// What a call says of itself: its unit's name, the tail of the "not what ... say" message, the text when the index is refused (a
// front may replace it in RD_JUDGE), and where its stats go.
struct rd_call {
    const char* unit; const char* not_what; const char* index_bad;
    uint64_t* decoded; uint32_t* waves_run;
};
// A call's front keeps a state of its own beside the shared one (rd.st) and goes where that goes: grown, cleared, filled between
// check and plan, read back in front of the one wait, judged behind it -- in front of the index's own verdict.
enum rd_step { RD_GROW, RD_CLEAR, RD_ENQUEUE, RD_READ, RD_JUDGE };
static dim3 rd_grid(uint64_t n) { return dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)); }

// Q holds the caller's side (source and its bound, index, reads); the workspace's side is filled here. front(step, Q) -> code;
// wave(Q, t0, t1, enqueue) -> code: the decode of the touched ranks [t0, t1) onto the stage, rooms and lengths into mem.caps /
// mem.out_lens, statuses into rd.status; enqueue == false: only grow what a wave of t1 - t0 ranks needs.
template <class Front, class Wave>
static int dec_reads(zz_ctx* c, hipStream_t st, zz_mr_params Q, rd_call& N, Front front, Wave wave)
{
    auto& R = c->dec.rd;
    auto& M = c->dec.mem;
    *N.decoded = 0; *N.waves_run = 0;
    const uint64_t entries = Q.entries, nranges = Q.nranges;
    if (int rc = R.st.grow(1)) return rc;
    if (int rc = R.h_st.grow(1)) return rc;
    if (int rc = front(RD_GROW, Q)) return rc;
    if (int rc = R.reads.grow(nranges)) return rc;
    if (int rc = R.chunk0.grow(nranges + 1)) return rc;
    if (int rc = R.diff.grow(entries)) return rc;
    if (int rc = R.cnt.grow(entries)) return rc;
    if (int rc = R.tlist.grow(entries)) return rc;
    if (int rc = R.S.grow(entries)) return rc;
    if (int rc = R.F.grow(entries)) return rc;
    if (int rc = R.G.grow(entries)) return rc;
    Q.reads = R.reads; Q.chunk0 = R.chunk0; Q.diff = R.diff; Q.cnt = R.cnt; Q.tlist = R.tlist; Q.S = R.S; Q.F = R.F; Q.G = R.G;
    Q.stage = nullptr; Q.st = R.st;

    // check, front, plan, touched: one readback
    HIPCHK(hipMemsetAsync(R.st, 0, sizeof(zz_mr_state), st));
    if (int rc = front(RD_CLEAR, Q)) return rc;
    HIPCHK(hipMemsetAsync(R.diff, 0, entries * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_mr_check, rd_grid(entries), dim3(256), 0, st, Q);
    if (int rc = front(RD_ENQUEUE, Q)) return rc;
    hipLaunchKernelGGL(k_mr_plan, rd_grid(nranges), dim3(256), 0, st, Q);
    hipLaunchKernelGGL(k_mr_touched, dim3(1), dim3(ZZ_MR_SCAN_THREADS), 0, st, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(R.h_st, R.st, sizeof(zz_mr_state), hipMemcpyDeviceToHost, st));
    if (int rc = front(RD_READ, Q)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = front(RD_JUDGE, Q)) return rc;
    if (R.h_st->index_bad) { set_err(N.index_bad); return ZZ_E_DATA; }
    const uint64_t touched = R.h_st->touched, nwaves = R.h_st->nwaves;
    if (touched) {
        // the waves' first ranks and S there: one readback
        if (int rc = R.waves.grow(2 * (nwaves + 1))) return rc;
        if (int rc = R.h_waves.grow(2 * (nwaves + 1))) return rc;
        hipLaunchKernelGGL(k_mr_waves, rd_grid(nwaves + 1), dim3(256), 0, st, Q, nwaves, (uint64_t*)R.waves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(R.h_waves, R.waves, 2 * (nwaves + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const uint64_t* W = R.h_waves.p;
        uint64_t big_items = 0, big_bytes = 0;
        for (uint64_t w = 0; w < nwaves; ++w) {
            big_items = std::max(big_items, W[2 * w + 2] - W[2 * w]);
            big_bytes = std::max(big_bytes, W[2 * w + 3] - W[2 * w + 1]);
        }
        if (int rc = R.stage.grow(big_bytes + 16)) return rc;
        if (int rc = wave(Q, 0, big_items, false)) return rc;
        if (int rc = R.status.grow(big_items)) return rc;
        Q.stage = R.stage;
        for (uint64_t w = 0; w < nwaves; ++w) {
            const uint64_t t0 = W[2 * w], t1 = W[2 * w + 2];
            if (t1 <= t0) continue;                                     // (cannot happen: a room is at most one wave's)
            ++*N.waves_run;
            if (int rc = wave(Q, t0, t1, true)) return rc;
            hipLaunchKernelGGL(k_mr_judge, dim3(1), dim3(ZZ_MR_SCAN_THREADS), 0, st, Q, t0, t1, (const uint64_t*)M.caps, (const uint64_t*)M.out_lens,
                               (const int32_t*)R.status);
            hipLaunchKernelGGL(k_mr_cut, dim3(1), dim3(ZZ_MR_SCAN_THREADS), 0, st, Q, t0, t1);
            hipLaunchKernelGGL(k_mr_copy, dim3(ZZ_MR_COPY_GRID), dim3(256), 0, st, Q, t0, t1);
            HIPCHK(hipGetLastError());
        }
        *N.decoded = touched - R.h_st->big;
    }
    hipLaunchKernelGGL(k_mr_verdict, rd_grid(nranges), dim3(256), 0, st, Q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(R.h_st, R.st, sizeof(zz_mr_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const zz_mr_state& T = *R.h_st.p;
    const std::string touch = std::string(" touch a ") + N.unit;
    if (T.n_data) { set_err("reads: " + std::to_string(T.n_data) + touch + " that is not what " + N.not_what); return ZZ_E_DATA; }
    if (T.n_unsupported) { set_err("reads: " + std::to_string(T.n_unsupported) + touch + " whose room exceeds the stage (64 MiB)"); return ZZ_E_UNSUPPORTED; }
    if (T.n_arg) { set_err("reads: " + std::to_string(T.n_arg) + " start behind the decoded length or overflow"); return ZZ_E_ARG; }
    if (T.n_nospace) { set_err("reads: " + std::to_string(T.n_nospace) + " do not fit their destinations"); return ZZ_E_NOSPACE; }
    return ZZ_OK;
}

extern "C" int zz_decode_members_ranges_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, const uint64_t* d_index, uint64_t entries,
                                               uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                               void* const* d_dsts, const uint64_t* d_caps,
                                               uint64_t* d_out_lens, int32_t* d_status, void* hip_stream)
{
    if (!c || !d_src_v || !d_index || !d_firsts || !d_nbytes || !d_dsts || !d_caps || !d_out_lens) { set_err("null argument"); return ZZ_E_ARG; }
    if (entries < 2) { set_err("the index needs at least two entries (members + 1)"); return ZZ_E_ARG; }
    if (entries - 1 > 0x7fffffffull) { set_err("at most 2^31 - 1 members per index"); return ZZ_E_ARG; }
    if (nranges > 0x7fffffffull) { set_err("at most 2^31 - 1 reads per call"); return ZZ_E_ARG; }
    if (nranges == 0) return ZZ_OK;                                 // nothing to do: the context is not looked at
    if (call_pending(c)) return ZZ_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& M = c->dec.mem;
    zz_mr_params Q;
    Q.src = (const uint8_t*)d_src_v; Q.src_len = src_len; Q.idx = d_index; Q.entries = entries;
    Q.nranges = nranges; Q.firsts = d_firsts; Q.nbytes = d_nbytes; Q.dsts = (uint8_t* const*)d_dsts; Q.caps = d_caps;
    Q.out_lens = d_out_lens; Q.status = d_status;
    rd_call N{ "member", "the index says",
               "reads: all fail, the index is not an index of this file (decoded offsets from 0 ascending, file offsets strictly ascending and inside the source)",
               &c->dec.mr.decoded, &c->dec.mr.waves_run };
    return dec_reads(c, st, Q, N, [](rd_step, const zz_mr_params&) { return ZZ_OK; },               // (no front)
        [&](const zz_mr_params& Q, uint64_t t0, uint64_t t1, bool enqueue) -> int {
            if (!enqueue) return ensure_member_items(c, t1 - t0);
            // descriptors from the index, then k_inflate_items as zz_decode_batch_device launches it
            hipLaunchKernelGGL(k_mr_desc, rd_grid(t1 - t0), dim3(256), 0, st, Q, t0, t1, (const uint8_t**)M.srcs.p, (uint64_t*)M.src_lens,
                               (uint8_t**)M.dsts.p, (uint64_t*)M.caps);
            HIPCHK(hipGetLastError());
            return dec_items(c, member_items_params(c, (uint32_t)(t1 - t0), c->dec.rd.status), st);
        });
}
extern "C" int zz_ctx_last_decode_members_ranges_stats(const zz_ctx* c, uint64_t* members_decoded, uint32_t* waves)
{
    if (!c) { set_err("null context"); return ZZ_E_ARG; }
    if (members_decoded) *members_decoded = c->dec.mr.decoded;
    if (waves) *waves = c->dec.mr.waves_run;
    return ZZ_OK;
}

// ---- reads of any stream through a point index with windows (zz_inflate_points_ranges.h; the rules in zz_inflate_core.h) ------
// The sidecar's builder: a second sequential pass on the host over a stream and an index of it, no GPU, no context.
extern "C" int zz_points_windows_host(const uint8_t* src, uint64_t src_len, int format, const uint64_t* points, uint64_t entries,
                                      uint8_t* windows, uint32_t* sums)
{
    if (!src || !points || !windows || !sums) { set_err("null argument"); return ZZ_E_ARG; }
    if (entries < 2) { set_err("a point index has at least two rows"); return ZZ_E_ARG; }
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    std::vector<uint8_t> ring(ZI_RING);
    std::vector<zi_tables> S(1);
    std::vector<zi_sum> sum(1);
    const int rc = zi_points_windows_build(src, src_len, format, points, entries, windows, sums, ring.data(), S[0], sum[0]);
    if (rc == ZI_ITEM_UNSUPPORTED) { set_err("the stream needs a preset dictionary (FDICT): not supported"); return ZZ_E_UNSUPPORTED; }
    if (rc) { set_err("not a valid stream of the requested format, or not an index of it (a row is no block boundary with its bytes in front of it)"); return ZZ_E_DATA; }
    return ZZ_OK;
}

// The same sidecar built on the device (zz_inflate_points_windows.h). A UNIT is what lies on the stage at once: the decode
// rows [g0, g1] -- decoded by dec_points_batch, in several launches where they are more than ZZ_PT_BATCH_SEGMENTS -- and the rows the
// cut works on: the sidecar's rows of a batch planned over `points`, or, for a sidecar segment longer than the stage, the two ends of
// a piece of it.
struct pw_unit {
    uint64_t g0, g1;                            // decode rows
    const uint64_t* cut_rows; uint32_t ncut;    // ncut + 1 rows (host): slots and sums of the segments between them
    uint8_t* win_dst; uint32_t* sum_dst;        // where slot 0 .. ncut - 1 and the sums go
    uint8_t* tail_dst;                          // where the slot of row ncut goes: the next unit's carry (null: the stream ends here)
};
static int pw_run_unit(zz_ctx* c, const uint8_t* s, uint64_t sn, const uint64_t* dec, uint64_t dec_entries, const pw_unit& U, uint8_t* d_dst,
                       uint64_t stage_bytes, int kind, hipStream_t st)
{
    auto& W = c->dec.pw;
    const uint64_t base = dec[2 * U.g0 + 1], end = dec[2 * U.g1 + 1];
    const int64_t org = zi_pw_org(base, d_dst != nullptr);
    uint8_t* const buf = d_dst ? d_dst : (uint8_t*)W.stage;
    uint8_t* const pos0 = (uint8_t*)((uintptr_t)buf - (uintptr_t)org);          // where position 0 would lie: the decode addresses by position
    for (uint64_t h0 = U.g0, h1; h0 < U.g1; h0 = h1) {
        h1 = zi_points_batches(dec, U.g1 + 1, h0, stage_bytes, ZZ_PT_BATCH_SEGMENTS);
        const int got = dec_points_batch(c, s, sn, dec + 2 * h0, (uint32_t)(h1 - h0), h1 + 1 == dec_entries, pos0, st, &W.pending, &W.rounds);
        if (got < 0) return got;
        if (got != DEC_DONE) { set_err("not an index of this stream: a segment does not decode from its row to the next with its bytes"); return ZZ_E_DATA; }
        ++W.batches;
    }
    HIPCHK(hipMemcpyAsync(W.rows, U.cut_rows, (uint64_t)(U.ncut + 1) * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(W.next, 0, sizeof(unsigned int), st));
    zz_pw_params Q;
    Q.buf = buf; Q.buf_n = d_dst ? end : ZI_PR_WINDOW + (end - base); Q.org = org; Q.rows = W.rows; Q.nseg = U.ncut;
    Q.windows = U.win_dst; Q.sums = U.sum_dst; Q.tail = U.tail_dst; Q.kind = kind; Q.next = W.next;
    const uint64_t items = (uint64_t)U.ncut + (U.tail_dst ? 1 : 0), resident = 256ull * ZZ_PT_WG_PER_CU;
    hipLaunchKernelGGL(k_points_windows_cut, dim3((uint32_t)(items < resident ? items : resident)), dim3(ZZ_INF_THREADS), 0, st, Q);
    HIPCHK(hipGetLastError());
    if (U.tail_dst && !d_dst) HIPCHK(hipMemcpyAsync(W.stage, U.tail_dst, ZI_PR_WINDOW, hipMemcpyDeviceToDevice, st));   // the next carry
    return ZZ_OK;
}

extern "C" int zz_points_windows_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, const uint64_t* points, uint64_t entries,
                                        const uint64_t* fine_points, uint64_t fine_entries, void* d_windows_v, uint32_t* d_sums,
                                        void* d_dst_v, uint64_t cap, uint64_t stage_bytes, void* hip_stream)
{
    if (!c || !d_src_v || !points || !d_windows_v || !d_sums) { set_err("null argument"); return ZZ_E_ARG; }
    if (entries < 2) { set_err("a point index has at least two rows (host memory)"); return ZZ_E_ARG; }
    if (entries - 1 > 0x7fffffffull) { set_err("at most 2^31 - 1 segments per index"); return ZZ_E_ARG; }
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    if (stage_bytes > ZZ_INF_BATCH_BYTES) { set_err("stage_bytes is at most " + std::to_string(ZZ_INF_BATCH_BYTES)); return ZZ_E_ARG; }
    if (!d_dst_v && cap) { set_err("null buffer"); return ZZ_E_ARG; }
    if (fine_points && !zi_points_superset(points, entries, fine_points, fine_entries)) {
        set_err("fine_points must hold every row of points, and the same first and last row");
        return ZZ_E_ARG;
    }
    if (call_pending(c)) return ZZ_E_ARG;
    const uint64_t segments = entries - 1, L = points[2 * segments + 1];
    if (d_dst_v && cap < L) { set_err("destination too small for the decoded stream (" + std::to_string(L) + " bytes)"); return ZZ_E_NOSPACE; }
    const uint8_t* d_src = (const uint8_t*)d_src_v;
    uint8_t* const d_windows = (uint8_t*)d_windows_v;
    uint8_t* const d_dst = (uint8_t*)d_dst_v;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& W = c->dec.pw;
    W.batches = 0; W.pending = 0; W.rounds = 0;
    int64_t hl = 0;
    if (int rc = dec_container(d_src, src_len, format, st, &hl)) return rc;
    const uint64_t tl = (uint64_t)trailer_len(format), sn = src_len - hl - tl;
    const uint64_t stage = stage_bytes ? stage_bytes : ZZ_INF_BATCH_BYTES;
    const uint64_t* const dec = fine_points ? fine_points : points;                // the rows decoded with
    const uint64_t dec_entries = fine_points ? fine_entries : entries;
    if (!zi_points_check(points, entries, sn, ~0ull, ~0ull) || !zi_points_check(dec, dec_entries, sn, ~0ull, ~0ull) ||
        (points[2 * segments] + 7) / 8 != sn) {
        set_err("not an index of this stream: row 0 = (0, 0), bits strictly ascending, bytes ascending, the last row directly in front of the trailer");
        return ZZ_E_DATA;
    }
    if (!zi_points_check(dec, dec_entries, sn, ~0ull, stage)) { set_err("a segment is longer than the stage (stage_bytes)"); return ZZ_E_UNSUPPORTED; }
    // the workspace: nothing on the stage is longer than min(stage, L)
    const uint64_t most = std::max<uint64_t>(1, std::min(stage, L));
    if (int rc = c->dec.tot.grow(ZZ_TOT_SLOTS)) return rc;
    if (int rc = dec_points_workspace(c, most, std::min<uint64_t>(ZZ_PT_BATCH_SEGMENTS, dec_entries - 1))) return rc;
    if (!d_dst) if (int rc = W.stage.grow(ZI_PR_WINDOW + most)) return rc;
    if (int rc = W.spare.grow(2 * ZI_PR_WINDOW)) return rc;
    if (int rc = W.rows.grow(2 * (std::min<uint64_t>(ZZ_PT_BATCH_SEGMENTS, segments) + 1))) return rc;
    if (int rc = W.piece.grow(1)) return rc;
    if (int rc = W.next.grow(1)) return rc;
    const int kind = zi_sidecar_kind(format);
    std::vector<uint32_t> got;                                                     // a batch's sums, for the fold
    zi_pr_part all{ 0, 0 };
    uint64_t piece_rows[4];
    uint32_t joined = 0;
    uint64_t f0 = 0;                                                               // the decode row that is row k0
    for (uint64_t k0 = 0, k1; k0 < segments; k0 = k1) {
        k1 = zi_points_batches(points, entries, k0, stage, ZZ_PT_BATCH_SEGMENTS);
        uint64_t f1 = f0 + (k1 - k0);
        if (fine_points) for (f1 = f0 + 1; f1 + 1 < fine_entries && fine_points[2 * f1] != points[2 * k1]; ++f1) {}   // (the superset walk found the row; bits ascend strictly)
        uint8_t* const tail = k1 < segments ? d_windows + k1 * ZI_PR_WINDOW : nullptr;
        if (points[2 * k1 + 1] - points[2 * k0 + 1] <= stage) {
            const pw_unit U{ f0, f1, points + 2 * k0, (uint32_t)(k1 - k0), d_windows + k0 * ZI_PR_WINDOW, d_sums + k0, tail };
            if (int rc = pw_run_unit(c, d_src + hl, sn, dec, dec_entries, U, d_dst, stage, kind, st)) return rc;
            got.resize(k1 - k0);
            HIPCHK(hipMemcpyAsync(got.data(), d_sums + k0, (k1 - k0) * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (uint64_t k = k0; k < k1; ++k) {
                zi_pr_part p;
                if (!zi_pr_entry_part(kind, got[k - k0], points[2 * k + 3] - points[2 * k + 1], &p)) { set_err("a segment's sum is none its length can have"); return ZZ_E_DATA; }
                all = zi_pr_join(kind, all, p);
            }
        } else {
            // one sidecar segment longer than the stage, decoded with finer rows: piece by piece, the pieces' sums joined here
            zi_pr_part seg{ 0, 0 };
            for (uint64_t g0 = f0, g1; g0 < f1; g0 = g1) {
                g1 = zi_points_batches(dec, f1 + 1, g0, stage, ZZ_PT_BATCH_SEGMENTS);
                piece_rows[0] = dec[2 * g0]; piece_rows[1] = dec[2 * g0 + 1]; piece_rows[2] = dec[2 * g1]; piece_rows[3] = dec[2 * g1 + 1];
                const pw_unit U{ g0, g1, piece_rows, 1, g0 == f0 ? d_windows + k0 * ZI_PR_WINDOW : (uint8_t*)W.spare, W.piece,
                                 g1 == f1 ? tail : (uint8_t*)W.spare + ZI_PR_WINDOW };
                if (int rc = pw_run_unit(c, d_src + hl, sn, dec, dec_entries, U, d_dst, stage, kind, st)) return rc;
                uint32_t v = 0;
                HIPCHK(hipMemcpyAsync(&v, W.piece, 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                zi_pr_part p;
                if (!zi_pr_entry_part(kind, v, piece_rows[3] - piece_rows[1], &p)) { set_err("a piece's sum is none its length can have"); return ZZ_E_DATA; }
                seg = zi_pr_join(kind, seg, p);
            }
            joined = zi_pr_public(kind, seg);
            HIPCHK(hipMemcpyAsync(d_sums + k0, &joined, 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
            all = zi_pr_join(kind, all, seg);
        }
        f0 = f1;
    }
    uint8_t t[8] = { 0 };
    if (tl) HIPCHK(hipMemcpyAsync(t, d_src + src_len - tl, tl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (all.len != L || !zi_pr_trailer_ok(format, t, all)) { set_err("the segments' sums do not fold to the stream's trailer (checksum or ISIZE mismatch)"); return ZZ_E_DATA; }
    return ZZ_OK;
}

extern "C" int zz_ctx_last_points_windows_stats(const zz_ctx* c, uint64_t* batches, uint64_t* pending_bytes, uint32_t* rounds)
{
    if (!c) { set_err("null ctx"); return ZZ_E_ARG; }
    if (batches) *batches = c->dec.pw.batches;
    if (pending_bytes) *pending_bytes = c->dec.pw.pending;
    if (rounds) *rounds = c->dec.pw.rounds;
    return ZZ_OK;
}

extern "C" int zz_points_thin(const uint64_t* points, uint64_t entries, uint64_t spacing, uint64_t* out, uint64_t max_entries, uint64_t* out_entries)
{
    if (!points || !out_entries) { set_err("null argument"); return ZZ_E_ARG; }
    *out_entries = 0;
    if (entries < 2) { set_err("a point index has at least two rows"); return ZZ_E_ARG; }
    if (spacing == 0) { set_err("spacing must be at least 1"); return ZZ_E_ARG; }
    *out_entries = zi_points_thin(points, entries, spacing, nullptr, 0);
    if (!out || max_entries < *out_entries) { set_err("point index buffer too small"); return ZZ_E_NOSPACE; }
    zi_points_thin(points, entries, spacing, out, max_entries);
    return ZZ_OK;
}

extern "C" int zz_decode_points_ranges_device(zz_ctx* c, const void* d_src_v, uint64_t src_len, int format, const uint64_t* d_points,
                                              uint64_t entries, const void* d_windows, const uint32_t* d_sums,
                                              uint64_t nranges, const uint64_t* d_firsts, const uint64_t* d_nbytes,
                                              void* const* d_dsts, const uint64_t* d_caps,
                                              uint64_t* d_out_lens, int32_t* d_status, void* hip_stream)
{
    if (!c || !d_src_v || !d_points || !d_windows || !d_sums || !d_firsts || !d_nbytes || !d_dsts || !d_caps || !d_out_lens) { set_err("null argument"); return ZZ_E_ARG; }
    if (entries < 2) { set_err("the index needs at least two rows (segments + 1)"); return ZZ_E_ARG; }
    if (entries - 1 > 0x7fffffffull) { set_err("at most 2^31 - 1 segments per index"); return ZZ_E_ARG; }
    if (nranges > 0x7fffffffull) { set_err("at most 2^31 - 1 reads per call"); return ZZ_E_ARG; }
    if (!dec_format_ok(format)) return ZZ_E_ARG;
    if (nranges == 0) return ZZ_OK;                                 // nothing to do: the context is not looked at
    if (call_pending(c)) return ZZ_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    auto& R = c->dec.rd;
    auto& M = c->dec.mem;
    auto& X = c->dec.pr;
    zz_mr_params Q;
    Q.src = (const uint8_t*)d_src_v; Q.idx = d_points; Q.entries = entries;
    Q.src_len = src_len > (~0ull >> 3) ? ~0ull : 8 * src_len;       // k_mr_check's bound on the last row: a bit inside the source (k_pr_front is exact)
    Q.nranges = nranges; Q.firsts = d_firsts; Q.nbytes = d_nbytes; Q.dsts = (uint8_t* const*)d_dsts; Q.caps = d_caps;
    Q.out_lens = d_out_lens; Q.status = d_status;
    zz_pr_params P;
    P.src = (const uint8_t*)d_src_v; P.src_len = src_len; P.format = format; P.windows = (const uint8_t*)d_windows; P.sums = d_sums;
    P.ps = nullptr; P.rooms = nullptr; P.out_lens = nullptr; P.status = nullptr;
    rd_call N{ "segment", "index and sidecar say",
               "reads: all fail, the rows are not a point index (row 0 = (0, 0), bits strictly ascending, bytes ascending)",
               &X.decoded, &X.waves_run };
    return dec_reads(c, st, Q, N,
        [&](rd_step step, const zz_mr_params& Q) -> int {
            switch (step) {
            case RD_GROW:
                if (int rc = X.st.grow(1)) return rc;
                if (int rc = X.h_st.grow(1)) return rc;
                P.ps = X.st;
                break;
            case RD_CLEAR: HIPCHK(hipMemsetAsync(X.st, 0, sizeof(zz_pr_state), st)); break;
            case RD_ENQUEUE: hipLaunchKernelGGL(k_pr_front, dim3(1), dim3(ZZ_PR_FRONT_THREADS), 0, st, Q, P); break;
            case RD_READ: HIPCHK(hipMemcpyAsync(X.h_st, X.st, sizeof(zz_pr_state), hipMemcpyDeviceToHost, st)); break;
            case RD_JUDGE:
                if (X.h_st->dict) { set_err("the stream needs a preset dictionary (FDICT): not supported"); return ZZ_E_UNSUPPORTED; }
                if (X.h_st->refused)
                    N.index_bad = "reads: all fail, the container header is invalid, the last row does not end where the trailer begins, or the sums do not fold to the trailer";
                break;
            }
            return ZZ_OK;
        },
        [&](const zz_mr_params& Q, uint64_t t0, uint64_t t1, bool enqueue) -> int {
            if (!enqueue) {
                if (int rc = M.caps.grow(t1 - t0)) return rc;
                return M.out_lens.grow(t1 - t0);
            }
            // persistent wavefronts, at most what the CUs hold at once, deal the ranks from a counter
            P.rooms = M.caps; P.out_lens = M.out_lens; P.status = R.status;
            HIPCHK(hipMemsetAsync(&X.st.p->next, 0, sizeof(unsigned int), st));
            hipLaunchKernelGGL(k_inflate_segments_win, dim3((uint32_t)std::min<uint64_t>(t1 - t0, 256ull * ZZ_PT_WG_PER_CU)), dim3(ZZ_INF_THREADS), 0, st,
                               Q, P, t0, t1);
            return ZZ_OK;
        });
}
extern "C" int zz_ctx_last_decode_points_ranges_stats(const zz_ctx* c, uint64_t* segments_decoded, uint32_t* waves)
{
    if (!c) { set_err("null context"); return ZZ_E_ARG; }
    if (segments_decoded) *segments_decoded = c->dec.pr.decoded;
    if (waves) *waves = c->dec.pr.waves_run;
    return ZZ_OK;
}

// The reference's fan-out and join (WriteDeflateStream, zzflate.cpp:97-155: ranges -> std::async encoders -> in-order
// memmove) for data that is ALREADY RESIDENT on several GPUs of one process -- the north star's dataflow without
// torch.distributed. Shard i (contiguous ranges of one stream, in order, every shard but the last a whole number of
// packets) lives on the device of ctxs[i]; all shards are encoded concurrently, each on its own device and stream; as
// shard i finishes, its compressed bytes are pulled over xGMI (hipMemcpyPeerAsync) straight to their final offset in
// d_dst, which lives on the device of ctxs[0] (shard 0 is encoded in place there); the checksum partials are folded on
// the host (adler.cpp:5-15 / GF(2) shifts) and header and trailer are written around the stream. No bulk collective.
// ---- peer access for the pulls of zz_encode_multi_device ------------------------------------------------------------------
// hipMemcpyPeerAsync works with or without peer access; without it the copy is staged through host memory instead of going
// over xGMI. So: once per ordered device pair (src -> dst), ask hipDeviceCanAccessPeer and enable access both ways; the answer
// is kept, "already enabled" counts as enabled, and zz_debug_peer_state tells a caller (and the tests) what a pull will use.
static std::mutex g_peer_mu;
static signed char g_peer[64][64];          // [dst][src]: 0 unknown, 1 peer access enabled, -1 not available (copies are staged)
static int peer_prepare(int dst, int src)
{
    if (dst == src) return 1;
    if (dst < 0 || src < 0 || dst >= 64 || src >= 64) return -1;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    if (g_peer[dst][src] == 0) {
        int prev = 0;
        (void)hipGetDevice(&prev);
        bool ok = true;
        for (int dir = 0; dir < 2 && ok; ++dir) {                    // dst reads/writes src's memory and the other way round
            const int a = dir ? src : dst, b = dir ? dst : src;
            int can = 0;
            ok = hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can != 0 && hipSetDevice(a) == hipSuccess;
            if (!ok) (void)hipGetLastError();
            if (ok) {
                const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
                if (e != hipSuccess) (void)hipGetLastError();    // whatever it was: the thread's last-error word must not leak into the next launch check
                ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;             // (idempotent)
            }
        }
        (void)hipSetDevice(prev);
        g_peer[dst][src] = g_peer[src][dst] = ok ? 1 : -1;
    }
    return g_peer[dst][src];
}
// (not part of the public header) 1: pulls from `src` to `dst` go peer to peer; -1: staged through the host; 0: not asked yet
extern "C" int zz_debug_peer_state(int dst, int src)
{
    if (dst == src) return 1;
    if (dst < 0 || src < 0 || dst >= 64 || src >= 64) return -1;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    return g_peer[dst][src];
}
// (not part of the public header) how many of the last zz_encode_multi_device call's pulls (this thread) went peer to peer / were staged
static thread_local int tl_pulls_p2p = 0, tl_pulls_staged = 0;
extern "C" void zz_debug_last_pulls(int* p2p, int* staged) { if (p2p) *p2p = tl_pulls_p2p; if (staged) *staged = tl_pulls_staged; }

extern "C" int zz_encode_multi_device(zz_ctx* const* ctxs, int nshards, const void* const* d_src, const uint64_t* n,
                                      const uint64_t* halo, void* d_dst, uint64_t cap, uint64_t* out_len, int format, int level,
                                      uint32_t P)
{
    if (out_len) *out_len = ~0ull;
    if (!ctxs || nshards < 1 || !d_src || !n || !d_dst || !out_len) { set_err("null argument"); return ZZ_E_ARG; }
    if (format < 0 || format > 2) format = ZZ_DEFLATE;
    if (P == 0) P = ZZ_DEFAULT_PACKET;
    if (P > ZZ_MAX_PACKET_SIZE) { set_err("packet size must be 1..32768"); return ZZ_E_ARG; }
    for (int i = 0; i < nshards; ++i) {
        if (!ctxs[i]) { set_err("null context"); return ZZ_E_ARG; }
        for (int j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) { set_err("every shard needs a context of its own"); return ZZ_E_ARG; }
        if (i + 1 < nshards && n[i] % P) { set_err("every shard but the last must be a whole number of packets"); return ZZ_E_ARG; }
        if (i + 1 < nshards && n[i] == 0) { set_err("empty shard in front of the last one"); return ZZ_E_ARG; }
    }
    const int hl = header_len(format), tl = trailer_len(format);
    if (cap < (uint64_t)hl) { set_err("destination smaller than the container header"); return ZZ_E_NOSPACE; }
    uint8_t* dst = (uint8_t*)d_dst;
    zz_ctx* c0 = ctxs[0];
    // the pulls' way: peer access between the first device and every other one, asked for and enabled once per pair
    tl_pulls_p2p = tl_pulls_staged = 0;
    for (int i = 1; i < nshards; ++i) (void)peer_prepare(c0->device, ctxs[i]->device);
    // enqueue every shard on its own device and stream; nothing waits yet
    std::vector<uint64_t> bound(nshards);
    for (int i = 0; i < nshards; ++i) {
        zz_ctx* c = ctxs[i];
        HIPCHK(hipSetDevice(c->device));
        if (!c->s_enc) HIPCHK(hipStreamCreateWithFlags(&c->s_enc, hipStreamNonBlocking));
        bound[i] = zz_bound(n[i], ZZ_DEFLATE, level > 3 ? 3 : level, P);
        uint8_t* out = nullptr;
        uint64_t ocap = 0;
        if (i == 0) { out = dst + hl; ocap = cap - hl; }               // final place: offset known
        else { int rc = ensure_stage(c, 0, bound[i]); if (rc) return rc; out = c->stage_out; ocap = c->stage_out.cap; }
        int rc = zz_encode_shard_device_async(c, d_src[i], n[i], halo ? halo[i] : 0, i + 1 == nshards, out, ocap, format, level, P,
                                              (void*)c->s_enc);
        if (rc) {           // finish what was enqueued so far: the contexts stay usable
            for (int j = 0; j < i; ++j) { uint64_t w; (void)zz_encode_shard_finish(ctxs[j], &w, nullptr, format); }
            return rc;
        }
    }
    // in-order join: shard i's offset is the sum of the sizes in front of it
    uint64_t off = (uint64_t)hl;
    uint32_t acc = format == ZZ_ZLIB ? 1u : 0u;
    uint64_t total_in = 0;
    int err = ZZ_OK;
    std::string errmsg;
    for (int i = 0; i < nshards; ++i) {
        zz_ctx* c = ctxs[i];
        uint64_t w = 0; uint32_t part = 0;
        int rc = zz_encode_shard_finish(c, &w, &part, format);
        if (rc && !err) { err = rc; errmsg = g_err; }
        if (err) continue;                                            // keep finishing: no context is left with a pending call
        if (off + w + (uint64_t)tl > cap) { err = ZZ_E_NOSPACE; errmsg = "destination too small for the compressed stream"; continue; }
        if (i > 0 && w) {
            if (hipSetDevice(c->device) != hipSuccess ||
                hipMemcpyPeerAsync(dst + off, c0->device, c->stage_out, c->device, w, c->s_enc) != hipSuccess) {
                err = ZZ_E_HIP; errmsg = "hipMemcpyPeerAsync failed"; continue;
            }
            if (peer_prepare(c0->device, c->device) == 1) tl_pulls_p2p++; else tl_pulls_staged++;
        }
        acc = format == ZZ_ZLIB ? adler_combine(acc, part, n[i]) : format == ZZ_GZIP ? crc32_combine(acc, part, n[i]) : 0u;
        off += w;
        total_in += n[i];
    }
    for (int i = 1; i < nshards; ++i) {                               // the pulls have landed
        (void)hipSetDevice(ctxs[i]->device);
        if (hipStreamSynchronize(ctxs[i]->s_enc) != hipSuccess && !err) { err = ZZ_E_HIP; errmsg = "hipStreamSynchronize failed after the peer copies"; }
    }
    if (err) { set_err(errmsg); return err; }
    HIPCHK(hipSetDevice(c0->device));
    uint8_t hdr[10], trl[8];
    const int hn = zz_header(format, hdr), tn = zz_trailer(format, acc, total_in, trl);
    if (hn) HIPCHK(hipMemcpy(dst, hdr, (size_t)hn, hipMemcpyHostToDevice));
    if (tn) HIPCHK(hipMemcpy(dst + off, trl, (size_t)tn, hipMemcpyHostToDevice));
    *out_len = off + (uint64_t)tn;
    return ZZ_OK;
}

// ---- container pieces --------------------------------------------------------------------------------
extern "C" int zz_header(int format, uint8_t out[10])
{
    static const uint8_t gz[10] = { 0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xFF };   // zzflate.cpp:28
    if (format == ZZ_ZLIB) { out[0] = 0x78; out[1] = 0x01; return 2; }          // zzflate.cpp:30-36
    if (format == ZZ_GZIP) { memcpy(out, gz, 10); return 10; }
    return 0;
}
extern "C" int zz_trailer(int format, uint32_t v, uint64_t n, uint8_t out[8])   // zzflate.cpp:170-192
{
    if (format == ZZ_ZLIB) { out[0] = v >> 24; out[1] = v >> 16; out[2] = v >> 8; out[3] = v; return 4; }
    if (format == ZZ_GZIP) {
        uint32_t l = (uint32_t)n;
        for (int i = 0; i < 4; ++i) { out[i] = (uint8_t)(v >> (8 * i)); out[4 + i] = (uint8_t)(l >> (8 * i)); }
        return 8;
    }
    return 0;
}

// ---- host checksum utilities (adler.cpp / crc.cpp API; not on the encode path) ----------------------------
extern "C" uint32_t zz_adler32(uint32_t start, const uint8_t* p, uint64_t n)
{
    uint64_t a = start & 0xFFFF, b = start >> 16;
    while (n) {
        uint64_t k = n < 5552 ? n : 5552;
        for (uint64_t i = 0; i < k; ++i) { a += p[i]; b += a; }
        a %= ZZ_ADLER_MOD; b %= ZZ_ADLER_MOD;
        p += k; n -= k;
    }
    return (uint32_t)((b << 16) | a);
}
extern "C" uint32_t zz_adler32_combine(uint32_t first, uint32_t second, uint64_t len2) { return adler_combine(first, second, len2); }
extern "C" uint32_t zz_crc32(const uint8_t* p, uint64_t n, uint32_t start)
{
    static uint32_t tab[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int j = 0; j < 8; ++j) c = (c >> 1) ^ ((c & 1u) * ZZ_CRC_POLY);
            tab[i] = c;
        }
    });
    uint32_t c = ~start;
    for (uint64_t i = 0; i < n; ++i) c = (c >> 8) ^ tab[(c & 0xFF) ^ p[i]];
    return ~c;
}
extern "C" uint32_t zz_crc32_combine(uint32_t c1, uint32_t c2, uint64_t len2) { return crc32_combine(c1, c2, len2); }

// ---- host-buffer entry points: contexts, devices -----------------------------------------------------------------
// The reference's entry points are re-entrant and, with threaded=true, fan the input out over every core of the
// machine (zzflate.cpp:97-132). Here a call borrows one context per device it uses from a small pool (created on
// demand, at most two per device, so concurrent callers overlap without unbounded memory) and fans the input's slabs
// out over every visible GPU. Which devices: env ZZFLATE_DEVICES ("0,1,2" -- an index may repeat, which gives that GPU
// several pipelines -- or "all"), else env ZZFLATE_DEVICE (one index), else all of them. No lock is held while
// kernels run or callbacks are invoked, so a callback may call back into the library.
static std::mutex g_mu;
static std::condition_variable g_cv;
static uint32_t g_packet = 0;
struct pool_entry { zz_ctx* c; bool busy; };
// contexts the calling THREAD holds through host calls further up its stack (a callback that calls back into the
// library): such a call must never wait for the pool -- the contexts it would wait for may be its own, or belong to
// another thread whose callback is waiting the same way -- so it gets a temporary context beyond the cap instead.
static thread_local int tl_leases = 0;
static std::vector<pool_entry> g_pool;
static std::vector<int> g_devices;
#define ZZ_POOL_PER_DEVICE 2

extern "C" uint32_t zz_get_packet_size(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_packet == 0) {
        const char* e = getenv("ZZFLATE_PACKET_SIZE");
        long v = e ? atol(e) : 0;
        g_packet = (v >= 1 && v <= (long)ZZ_MAX_PACKET_SIZE) ? (uint32_t)v : ZZ_DEFAULT_PACKET;
    }
    return g_packet;
}
extern "C" int zz_set_packet_size(uint32_t P)
{
    if (P == 0 || P > ZZ_MAX_PACKET_SIZE) { set_err("packet size must be 1..32768"); return ZZ_E_ARG; }
    std::lock_guard<std::mutex> lk(g_mu);
    g_packet = P;
    return ZZ_OK;
}

// the device list of the host entry points (read once)
static int host_devices(std::vector<int>& out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_devices.empty()) {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count == 0) {
            set_err(std::string("no HIP device available (hipGetDeviceCount: ") + hipGetErrorString(e) + ", count " +
                    std::to_string(count) + "): this library has no CPU encode path");
            return ZZ_E_HIP;
        }
        const char* list = getenv("ZZFLATE_DEVICES");
        const char* one = getenv("ZZFLATE_DEVICE");
        std::vector<int> v;
        if (list && *list && strcmp(list, "all") != 0) {
            for (const char* q = list; *q;) {
                char* endp = nullptr;
                const long d = strtol(q, &endp, 10);
                if (endp == q) break;
                if (d < 0 || d >= count) { set_err("ZZFLATE_DEVICES names a device that does not exist"); return ZZ_E_ARG; }
                v.push_back((int)d);
                q = *endp == ',' ? endp + 1 : endp;
            }
        } else if (!list && one && *one) {
            const int d = atoi(one);
            if (d < 0 || d >= count) { set_err("ZZFLATE_DEVICE names a device that does not exist"); return ZZ_E_ARG; }
            v.push_back(d);
        }
        if (v.empty()) for (int d = 0; d < count; ++d) v.push_back(d);
        g_devices = v;
    }
    out = g_devices;
    return ZZ_OK;
}
// test hook (not in the public header): forget the device list so that the environment is read again
extern "C" void zz_debug_reset_devices(void) { std::lock_guard<std::mutex> lk(g_mu); g_devices.clear(); }

// `held`: contexts of this device the calling host call already holds (ZZFLATE_DEVICES may name a device several
// times). A call only ever waits for its first context of a device, devices are taken in one global order, and a
// `nested` call (its thread holds contexts through calls further up its stack) never waits at all: concurrent and
// nested calls cannot block each other for good.
// *temp = the context was created beyond the cap for a nested call and is destroyed on release.
static int pool_acquire(int device, int held, bool nested, zz_ctx** out, bool* temp)
{
    *temp = false;
    std::unique_lock<std::mutex> lk(g_mu);
    for (;;) {
        int have = 0;
        static const uint32_t warm = [] {               // env ZZFLATE_WARM_WINDOW: warm window of the host entry points
            const char* e = getenv("ZZFLATE_WARM_WINDOW");
            const long v = e ? atol(e) : 0;
            return (uint32_t)(v < 0 ? 0 : v > 32768 ? 32768 : v);
        }();
        static const bool ext = [] { const char* e = getenv("ZZFLATE_EXTENDED_LEVELS"); return e && atoi(e) != 0; }();
        if ((warm || ext) && !lds_order_ok(device)) {   // (the same refusal as zz_ctx_set_warm_window / zz_ctx_set_extended_levels)
            set_err("ZZFLATE_WARM_WINDOW / ZZFLATE_EXTENDED_LEVELS refused: this device's LDS does not serve equal addresses in lane order");
            return ZZ_E_UNSUPPORTED;
        }
        for (auto& e : g_pool)
            if (e.c->device == device) {
                if (!e.busy) { e.busy = true; e.c->warm = warm; e.c->extended = ext; *out = e.c; return ZZ_OK; }
                have++;
            }
        if (have < ZZ_POOL_PER_DEVICE + held || nested) {
            zz_ctx* c = nullptr;
            int rc = zz_ctx_create(device, &c);
            if (rc) return rc;
            c->warm = warm; c->extended = ext;
            if (have < ZZ_POOL_PER_DEVICE + held) g_pool.push_back({ c, true });
            else *temp = true;
            *out = c;
            return ZZ_OK;
        }
        g_cv.wait(lk);
    }
}
static void pool_release(zz_ctx* c)
{
    { std::lock_guard<std::mutex> lk(g_mu); for (auto& e : g_pool) if (e.c == c) e.busy = false; }
    g_cv.notify_all();
}
struct ctx_lease {                       // contexts borrowed for one host call
    std::vector<zz_ctx*> v;
    std::vector<bool> temp;
    const int outer = tl_leases;         // contexts held by host calls further up this thread's stack
    ~ctx_lease()
    {
        for (size_t i = 0; i < v.size(); ++i) { if (temp[i]) zz_ctx_destroy(v[i]); else pool_release(v[i]); }
        tl_leases -= (int)v.size();
    }
    int take(int device)
    {
        int held = 0;
        for (zz_ctx* h : v) held += h->device == device;
        zz_ctx* c = nullptr;
        bool t = false;
        int rc = pool_acquire(device, held, outer > 0, &c, &t);
        if (!rc) { v.push_back(c); temp.push_back(t); tl_leases++; }
        return rc;
    }
};

// ---- host-buffer entry points ------------------------------------------------------------------------------------
// Where the compressed bytes go: straight into the caller's destination (ZzFlateEncode, zzflate.cpp:225-242) or
// through the callback in library-owned chunks (ZzFlateEncodeToCallback, zzflate.cpp:197-222): at most 1,000,000 bytes
// each (outputbitstream.h:183); header and trailer are calls of their own, as in the reference.
struct host_sink {
    // destination form
    uint8_t* dest = nullptr; uint64_t cap = 0, pos = 0; bool overflow = false;
    // callback form
    zz_callback cb = nullptr; void* user = nullptr; std::vector<uint8_t> chunk;
    void raw(const uint8_t* p, uint64_t n)            // header / trailer / a chunk with the reference's own boundaries
    {
        if (cb) { flush(); cb(user, p, n); return; }          // also for 0 bytes (raw deflate: zzflate.cpp:205,221 call regardless)
        put(p, n);
    }
    void put(const uint8_t* p, uint64_t n)            // stream bytes
    {
        if (!cb) {
            if (overflow || n > cap - pos) { overflow = true; return; }
            memcpy_mt(dest + pos, p, n);
            pos += n;
            return;
        }
        while (n) {
            const uint64_t room = 1000000 - chunk.size();
            const uint64_t k = n < room ? n : room;
            chunk.insert(chunk.end(), p, p + k);
            p += k; n -= k;
            if (chunk.size() == 1000000) flush();
        }
    }
    void flush() { if (cb && !chunk.empty()) { cb(user, chunk.data(), chunk.size()); chunk.clear(); } }
    static void memcpy_mt(uint8_t* d, const uint8_t* s, uint64_t n)
    {
        // pageable <-> pinned copies of whole slabs: a few threads reach the memory bandwidth one thread cannot
        const uint64_t piece = 8ull << 20;
        if (n < 2 * piece) { memcpy(d, s, n); return; }
        const unsigned nt = (unsigned)((n + piece - 1) / piece < 8 ? (n + piece - 1) / piece : 8);
        const uint64_t per = ((n + nt - 1) / nt + 4095) & ~4095ull;
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) {
            const uint64_t o = (uint64_t)t * per;
            if (o >= n) break;
            th.emplace_back([=] { memcpy(d + o, s + o, n - o < per ? n - o : per); });
        }
        memcpy(d, s, per < n ? per : n);
        for (auto& x : th) x.join();
    }
};

static uint64_t slab_bytes(uint32_t P)
{
    uint64_t mib = 64;
    if (const char* e = getenv("ZZFLATE_SLAB_MIB")) { const long v = atol(e); if (v >= 1 && v <= 4096) mib = (uint64_t)v; }
    const uint64_t s = mib << 20;
    return s < P ? P : s / P * P;          // slabs are cut at packet boundaries
}

// bytes of input kept in front of a slab on the device: level >= 2 extends matches backward over at most 258 bytes
// (encoder.cpp:92-102,404, capped as D11 says) and compares eight at a time; a warm window reaches back 32768
#define ZZ_SLAB_HALO 36864ull

static int ensure_pipe(zz_ctx* c, uint64_t slab, uint64_t slab_bound)
{
    if (!c->s_in) {
        HIPCHK(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&c->s_enc, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIPCHK(hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
        }
    }
    // each pair is freed before any of it is allocated again; the test is on the buffer allocated last, so that a failure half way
    // starts over on the next call
    const uint64_t in_bytes = ZZ_SLAB_HALO + slab;
    if (in_bytes + 64 > c->slab_in[1].cap) {
        for (int i = 0; i < 2; ++i) { c->pin_in[i].release(); c->slab_in[i].release(); }
        for (int i = 0; i < 2; ++i) {
            if (int rc = c->pin_in[i].grow(in_bytes)) return rc;
            if (int rc = c->slab_in[i].grow(in_bytes + 64)) return rc;
        }
    }
    if (slab_bound + 64 > c->slab_out[1].cap) {
        for (int i = 0; i < 2; ++i) { c->pin_out[i].release(); c->slab_out[i].release(); }
        for (int i = 0; i < 2; ++i) {
            if (int rc = c->pin_out[i].grow(slab_bound)) return rc;
            if (int rc = c->slab_out[i].grow(slab_bound + 64)) return rc;
        }
    }
    return ZZ_OK;
}

// Packet mode on a host buffer (SURVEY.md 8f.1 and the device analogue of the std::async fan-out, zzflate.cpp:97-155).
// The input is cut into slabs of whole packets; slab i belongs to device i mod D. Every device runs its own pipeline
// on its own host thread: the slab crosses PCIe (through a pinned buffer) while the device's previous slab is encoded
// as a shard of the stream (no container; checksum partial returned) and the one before that travels back. Only two
// slabs of input -- each with the 4 KiB in front of it, for level >= 2's backward match extension -- and two of output
// live on a device at any time, so the input may be far larger than HBM. The calling thread is the in-order join: it
// hands the slabs' bytes to the sink as they arrive and folds the checksum partials (adler.cpp:5-15 / GF(2) shifts).
static int encode_host_slabs(const std::vector<zz_ctx*>& ctxs, const uint8_t* src, uint64_t n, int format, int level, uint32_t P,
                             host_sink& sink)
{
    const uint64_t slab = slab_bytes(P);
    const uint64_t nslab = (n + slab - 1) / slab;
    const uint64_t sb = zz_bound(slab, ZZ_DEFLATE, level, P);
    const int D = (int)ctxs.size();
    const int ck = format == ZZ_ZLIB ? ZZ_ZLIB : format == ZZ_GZIP ? ZZ_GZIP : ZZ_DEFLATE;

    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint64_t> out_len(nslab, 0);
    std::vector<uint32_t> part(nslab, 0);
    std::vector<uint8_t> ready(nslab, 0), consumed(nslab, 0);
    int err = 0;
    std::string errmsg;
    auto fail = [&](int rc) {
        std::lock_guard<std::mutex> lk(mu);
        if (!err) { err = rc; errmsg = g_err; }
        cv.notify_all();
    };

    auto worker = [&](int d) {
        zz_ctx* c = ctxs[d];
        auto run = [&]() -> int {
            HIPCHK(hipSetDevice(c->device));
            int rc = ensure_pipe(c, slab, sb);
            if (rc) return rc;
            auto stage_in = [&](uint64_t j) -> int {                       // j: this device's j-th slab
                const uint64_t i = (uint64_t)d + j * D, off = i * slab, len = n - off < slab ? n - off : slab;
                const uint64_t h = off < ZZ_SLAB_HALO ? off : ZZ_SLAB_HALO;
                const int b = (int)(j & 1);
                // pin_in[b] / slab_in[b] were last used by slab j-2, whose encode has returned
                host_sink::memcpy_mt(c->pin_in[b] + ZZ_SLAB_HALO - h, src + off - h, h + len);
                HIPCHK(hipMemcpyAsync(c->slab_in[b] + ZZ_SLAB_HALO - h, c->pin_in[b] + ZZ_SLAB_HALO - h, h + len, hipMemcpyHostToDevice, c->s_in));
                HIPCHK(hipEventRecord(c->ev_in[b], c->s_in));
                return ZZ_OK;
            };
            const uint64_t mine = nslab > (uint64_t)d ? (nslab - d + D - 1) / D : 0;
            if (mine == 0) return ZZ_OK;
            rc = stage_in(0);
            if (rc) return rc;
            for (uint64_t j = 0; j < mine; ++j) {
                const uint64_t i = (uint64_t)d + j * D, off = i * slab, len = n - off < slab ? n - off : slab;
                const uint64_t h = off < ZZ_SLAB_HALO ? off : ZZ_SLAB_HALO;
                const int b = (int)(j & 1);
                if (j + 1 < mine) { rc = stage_in(j + 1); if (rc) return rc; }     // the next slab's copy runs under this slab's encode
                HIPCHK(hipStreamWaitEvent(c->s_enc, c->ev_in[b], 0));
                if (j >= 2) {
                    // the output buffers of slab j-2: its copy back must be over, and the join must have taken the bytes
                    HIPCHK(hipStreamWaitEvent(c->s_enc, c->ev_out[b], 0));
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return err || consumed[i - 2 * (uint64_t)D]; });
                    if (err) return ZZ_OK;
                }
                uint64_t w = 0; uint32_t pc = 0;
                rc = zz_encode_shard_device(c, c->slab_in[b] + ZZ_SLAB_HALO, len, h, i + 1 == nslab, c->slab_out[b], c->pin_out[b].cap, &w, &pc,
                                            ck, level, P, (void*)c->s_enc);     // returns when the slab is encoded
                if (rc) return rc;
                HIPCHK(hipMemcpyAsync(c->pin_out[b], c->slab_out[b], w, hipMemcpyDeviceToHost, c->s_out));
                HIPCHK(hipEventRecord(c->ev_out[b], c->s_out));              // the join waits for it; this thread moves on
                {
                    std::lock_guard<std::mutex> lk(mu);
                    out_len[i] = w; part[i] = pc; ready[i] = 1;
                }
                cv.notify_all();
                { std::lock_guard<std::mutex> lk(mu); if (err) return ZZ_OK; }
            }
            return ZZ_OK;
        };
        const int rc = run();
        if (rc) fail(rc);
    };

    std::vector<std::thread> threads;
    for (int d = 0; d < D; ++d) threads.emplace_back(worker, d);
    uint8_t hdr[10], trl[8];
    uint32_t acc = format == ZZ_ZLIB ? 1u : 0u;          // running checksum of everything in front of the slab
    for (uint64_t i = 0; i < nslab; ++i) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return err || ready[i]; });
            if (err) break;
        }
        if (i == 0) sink.raw(hdr, (uint64_t)zz_header(format, hdr));    // nothing is delivered before a slab has encoded
        const uint64_t off = i * slab, len = n - off < slab ? n - off : slab;
        zz_ctx* c = ctxs[i % D];
        const int b = (int)((i / D) & 1);
        if (hipEventSynchronize(c->ev_out[b]) != hipSuccess) { set_err("hipEventSynchronize failed in the slab join"); fail(ZZ_E_HIP); break; }
        sink.put(c->pin_out[b], out_len[i]);
        acc = format == ZZ_ZLIB ? adler_combine(acc, part[i], len) : format == ZZ_GZIP ? crc32_combine(acc, part[i], len) : 0u;
        { std::lock_guard<std::mutex> lk(mu); consumed[i] = 1; }
        cv.notify_all();
    }
    for (auto& t : threads) t.join();
    if (err) { set_err(errmsg); return err; }
    sink.raw(trl, (uint64_t)zz_trailer(format, acc, n, trl));
    sink.flush();
    return ZZ_OK;
}

// one slab or less: one copy in, one call, one copy out
static int encode_host_simple(zz_ctx* c, const uint8_t* src, uint64_t n, int format, int level, uint32_t P, host_sink& sink)
{
    const uint64_t bound = zz_bound(n, format, level, P);
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_stage(c, n, bound);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpy(c->stage_in, src, n, hipMemcpyHostToDevice));
    uint64_t total = 0;
    rc = zz_encode_device(c, c->stage_in, n, c->stage_out, bound, &total, format, level, P, nullptr);
    if (rc) return rc;
    std::vector<uint8_t> host(total);
    if (total) HIPCHK(hipMemcpy(host.data(), c->stage_out, total, hipMemcpyDeviceToHost));
    const uint64_t hl = header_len(format), tl = trailer_len(format);
    sink.raw(host.data(), hl);
    sink.put(host.data() + hl, total - hl - tl);
    sink.raw(host.data() + total - tl, tl);
    sink.flush();
    return ZZ_OK;
}

// threaded == false: the reference's single Encoder over the whole input (zzflate.cpp:84-95). Its output depends on
// where it goes: into the caller's buffer the level-1 block lengths follow from the buffer's size; through the callback
// they follow from the library's own 1,000,000-byte chunks, and the callback sees exactly those chunks.
static int encode_host_sequential(zz_ctx* c, const uint8_t* src, uint64_t n, int format, int level, host_sink& sink)
{
    const bool chunked = sink.cb != nullptr;
    const uint64_t hl = header_len(format), tl = trailer_len(format);
    // device buffer for the stream: level 1 never needs more than nine bits per byte plus ten per block
    uint64_t bound = zz_bound(n, format, level, ZZ_DEFAULT_PACKET) + n / 65536 + 256;
    uint64_t cap = bound;
    if (!chunked && level == 1 && sink.cap < cap) cap = sink.cap;      // the caller's capacity decides the block lengths
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_stage(c, n, cap > bound ? cap : bound);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpy(c->stage_in, src, n, hipMemcpyHostToDevice));
    zz_result r;
    std::vector<uint64_t> chunks;
    rc = encode_stream(c, c->stage_in, n, c->stage_out, cap, format, level, chunked, chunked ? &chunks : nullptr, nullptr, &r);
    if (rc) return rc;
    const uint64_t total = r.total_bytes;
    std::vector<uint8_t> host(total);
    if (total) HIPCHK(hipMemcpy(host.data(), c->stage_out, total, hipMemcpyDeviceToHost));
    sink.raw(host.data(), hl);
    if (chunked) {
        uint64_t o = hl;
        for (uint64_t k : chunks) { sink.raw(host.data() + o, k); o += k; }   // one call per chunk (zzflate.cpp:207-215)
    } else {
        sink.put(host.data() + hl, total - hl - tl);
    }
    sink.raw(host.data() + total - tl, tl);
    sink.flush();
    return ZZ_OK;
}

// ZZFLATE_RANGES=<count>, threaded != 0, levels 0, 2, 3: the reference's own split (encode_ranges) instead of packets
static int encode_host_ranges(zz_ctx* c, const uint8_t* src, uint64_t n, int format, int level, uint32_t count, host_sink& sink)
{
    const uint64_t hl = header_len(format), tl = trailer_len(format);
    const uint64_t bound = n + (n / 65535 + 2 * (uint64_t)count + 2) * 5 + (n / 400000 + 2 * (uint64_t)count + 2) * 8 + 6ull * count + 64 + hl + tl;
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_stage(c, n, bound);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpy(c->stage_in, src, n, hipMemcpyHostToDevice));
    zz_result r;
    rc = encode_ranges(c, c->stage_in, n, c->stage_out, bound, format, level, count, nullptr, &r);
    if (rc) return rc;
    const uint64_t total = r.total_bytes;
    std::vector<uint8_t> host(total);
    if (total) HIPCHK(hipMemcpy(host.data(), c->stage_out, total, hipMemcpyDeviceToHost));
    sink.raw(host.data(), hl);
    sink.put(host.data() + hl, total - hl - tl);
    sink.raw(host.data() + total - tl, tl);
    sink.flush();
    return ZZ_OK;
}

static int encode_host(const uint8_t* src, uint64_t n, const zz_config* cfg, host_sink& sink)
{
    const int level = cfg->level;
    static const bool ext = [] { const char* e = getenv("ZZFLATE_EXTENDED_LEVELS"); return e && atoi(e) != 0; }();
    if (level < 0 || level > (ext ? 6 : 3)) { set_err("level must be 0..3"); return ZZ_E_LEVEL; }
    if (level > 3 && !cfg->threaded) { set_err("levels 4..6 exist in packet mode only (threaded != 0)"); return ZZ_E_LEVEL; }
    if (!src && n) { set_err("null source"); return ZZ_E_ARG; }
    std::vector<int> devs;
    int rc = host_devices(devs);
    if (rc) return rc;
    const uint32_t P = zz_get_packet_size();
    int format = cfg->format;
    if (format < 0 || format > 2) format = ZZ_DEFLATE;
    ctx_lease lease;
    if (!cfg->threaded && n > 0) {
        rc = lease.take(devs[0]);
        if (rc) return rc;
        return encode_host_sequential(lease.v[0], src, n, format, level, sink);
    }
    {
        const char* e = getenv("ZZFLATE_RANGES");                         // (read per call: tests switch it)
        const int count = e ? atoi(e) : 0;
        // (only where the split's preconditions hold -- count <= 4096, n < 2 GiB, every range inside the input; otherwise the
        // call is served in packet mode like any other: the environment switch must not turn working calls into errors)
        if (count > 0 && count <= 4096 && n > 0 && n < (1ull << 31) && level != 1 && level <= 3 &&
            (n < 100ull * (uint64_t)count || ranges_split_ok(n, (uint32_t)count))) {
            rc = lease.take(devs[0]);
            if (rc) return rc;
            return encode_host_ranges(lease.v[0], src, n, format, level, (uint32_t)count, sink);
        }
    }
    const uint64_t slab = slab_bytes(P);
    const uint64_t nslab = (n + slab - 1) / slab;
    if (nslab <= 1) {
        rc = lease.take(devs[0]);
        if (rc) return rc;
        return encode_host_simple(lease.v[0], src, n, format, level, P, sink);
    }
    const size_t D = devs.size() < nslab ? devs.size() : (size_t)nslab;
    for (size_t d = 0; d < D; ++d) { rc = lease.take(devs[d]); if (rc) return rc; }
    return encode_host_slabs(lease.v, src, n, format, level, P, sink);
}

extern "C" int zz_encode(uint8_t* dest, uint64_t* dest_len, const uint8_t* src, uint64_t n, const zz_config* cfg)
{
    if (!dest_len) { set_err("null dest_len"); return ZZ_E_ARG; }
    const uint64_t cap = *dest_len;
    *dest_len = ~0ull;
    if (!cfg || !dest) { set_err("null argument"); return ZZ_E_ARG; }
    if (cap < (uint64_t)header_len(cfg->format)) { set_err("destination smaller than the container header"); return ZZ_E_NOSPACE; }
    host_sink sink;
    sink.dest = dest; sink.cap = cap;
    const int rc = encode_host(src, n, cfg, sink);
    if (rc) return rc;
    if (sink.overflow) { set_err("destination too small for the compressed stream"); return ZZ_E_NOSPACE; }
    *dest_len = sink.pos;
    return ZZ_OK;
}

extern "C" int zz_encode_callback(const uint8_t* src, uint64_t n, const zz_config* cfg, zz_callback cb, void* user)
{
    if (!cfg || !cb) { set_err("null argument"); return ZZ_E_ARG; }
    host_sink sink;
    sink.cb = cb; sink.user = user;
    sink.chunk.reserve(1000000);
    return encode_host(src, n, cfg, sink);
}

// diagnostic (not in the public header): device bytes the host entry points' contexts hold for input/output staging
extern "C" uint64_t zz_debug_host_staging_bytes(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    uint64_t t = 0;
    for (auto& e : g_pool)
        t += e.c->stage_in.bytes() + e.c->stage_out.bytes() + e.c->slab_in[0].bytes() + e.c->slab_in[1].bytes() + e.c->slab_out[0].bytes() + e.c->slab_out[1].bytes();
    return t;
}

// ---- synthetic inputs -----------------------------------------------------------------------------------------
__global__ void k_generate(int kind, uint64_t seed, uint64_t first_block, uint8_t* buf, uint64_t n)
{
    uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t off = b * ZZ_GEN_BLOCK;
    if (off >= n) return;
    uint32_t cap = (uint32_t)(n - off < ZZ_GEN_BLOCK ? n - off : ZZ_GEN_BLOCK);
    zzgen::gen_block(kind, seed, first_block + b, buf + off, cap);
}

extern "C" int zz_generate_device(zz_ctx* c, int kind, uint64_t seed, uint64_t first_byte, void* d_buf, uint64_t n,
                                  void* hip_stream)
{
    if (!c || !d_buf) { set_err("null argument"); return ZZ_E_ARG; }
    if (first_byte % ZZ_GEN_BLOCK) { set_err("first_byte must be a multiple of 65536"); return ZZ_E_ARG; }
    if (n == 0) return ZZ_OK;
    HIPCHK(hipSetDevice(c->device));
    uint64_t nb = (n + ZZ_GEN_BLOCK - 1) / ZZ_GEN_BLOCK;
    hipLaunchKernelGGL(k_generate, dim3((uint32_t)((nb + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, kind, seed,
                       first_byte / ZZ_GEN_BLOCK, (uint8_t*)d_buf, n);
    HIPCHK(hipGetLastError());
    return ZZ_OK;
}
extern "C" int zz_generate_host(int kind, uint64_t seed, uint64_t first_byte, uint8_t* buf, uint64_t n)
{
    if (!buf) { set_err("null argument"); return ZZ_E_ARG; }
    if (first_byte % ZZ_GEN_BLOCK) { set_err("first_byte must be a multiple of 65536"); return ZZ_E_ARG; }
    for (uint64_t off = 0; off < n; off += ZZ_GEN_BLOCK) {
        uint32_t cap = (uint32_t)(n - off < ZZ_GEN_BLOCK ? n - off : ZZ_GEN_BLOCK);
        zzgen::gen_block(kind, seed, (first_byte + off) / ZZ_GEN_BLOCK, buf + off, cap);
    }
    return ZZ_OK;
}
