// inflate_points_harness.cpp -- CPU harness of the point-index decode (zzflate_amd/csrc/zz_inflate_core.h: ZI_RUN_POINT,
// zi_out_segment, zi_points_check, zi_points_batches, zi_points_build), the host restatement of zz_decode_points_device:
// the builder, the check, the batches, phase 1 per segment (k_inflate_segments), the tile counts (k_points_count), the rounds
// (k_inflate_resolve's rule, one round reading the state the round before left), the trailer's verdict and the serial path
// behind a refusal. tests/test_points_cases_cpu.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer
// access of the core checked; out of range aborts the process) and calls it through ctypes.
//
//   zpt_build(src, n, format, spacing, rows, max_entries, &entries, &out_len) -> status
//   zpt_decode(src, n, format, rows, entries, out, cap, batch_limit, lanes, &out_len, stats) -> status
//   zpt_segments_alone(src, n, format, rows, entries, data, data_len) -> segments that are not their slice of `data`
//
// Simulated lanes (lanes = 2..64), as in inflate_items_harness.cpp: every lane is a coroutine running the segment's zi_run with
// its own lane number over the SAME tables, destination, bitmap and pointers. A lane runs alone until it depends on what other
// lanes wrote -- ZI_LANES_SYNC() in the table builder, the out policy's fence in front of a copy -- and there the next lane runs,
// round robin: a barrier. Between two barriers the lanes repeat identical writes or write disjoint places, as on the device.
#define HARNESS_NAME "inflate_points_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

// one segment's phase 1, as k_inflate_segments sets it up
struct seg_call {
    zi_view<const uint8_t> view;               // the DEFLATE bytes (no trailer)
    uint64_t b0, o0, b1, o1; bool last;
    uint8_t* dst; uint64_t base, nbytes;
    uint32_t* st; uint32_t* pend; uint64_t words;
    zi_tables* S;
    zi_result res[MAX_LANES]; uint64_t end_bit[MAX_LANES]; uint32_t npend[MAX_LANES];
};
seg_call g_seg;

void lane_main(int lane)
{
    seg_call& c = g_seg;
    zi_in_mem in{ c.view };
    zi_out_segment<host_fence, zi_bits_plain> o{ zi_view<uint8_t>{ c.dst + c.o0, c.o1 - c.o0 }, zi_view<uint32_t>{ c.pend, c.words },
                                                 zi_view<uint32_t>{ c.st, c.nbytes }, c.o0, c.o0 - c.base, 0, 0, false, (uint32_t)lane,
                                                 g_nl, {}, {} };
    zi_pt_segment pt{ (uint32_t)(c.b0 & 7), c.b1, c.last, 0 };
    c.res[lane] = zi_run(in, c.view, c.b0 >> 3, o, *c.S, ZI_RUN_POINT, c.o1 - c.o0, (uint32_t)lane, g_nl, pt);
    c.end_bit[lane] = pt.end_bit;
    c.npend[lane] = o.npend;
}

// runs g_seg with `lanes` lanes; false: the lanes disagree (a harness failure)
bool run_segment(uint32_t lanes)
{
    memset(g_seg.S, 0xA5, sizeof *g_seg.S);                   // nothing may rely on what the tables held
    g_seg.S->kind = 0;
    if (!run_lanes(lanes, lane_main)) return false;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_seg.res[l].err != g_seg.res[0].err || g_seg.res[l].out != g_seg.res[0].out || g_seg.res[l].final != g_seg.res[0].final ||
            g_seg.end_bit[l] != g_seg.end_bit[0]) return false;
    return true;
}

struct row_sink { std::vector<uint64_t> rows; void put(uint64_t bit, uint64_t pos) { rows.push_back(bit); rows.push_back(pos); } };

uint64_t tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }

// the serial path and its verdict: what zz_decode_device(packet_size 0) answers
int serial(const uint8_t* src, uint64_t n, int format, uint8_t* out, uint64_t cap, uint64_t* out_len)
{
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return ZI_ITEM_UNSUPPORTED;
    if (hl < 0 || n - (uint64_t)hl < tlen(format)) return ZI_ITEM_DATA;
    std::vector<uint8_t> copy(src + hl, src + n);
    zi_view<const uint8_t> view{ copy.data(), copy.size() };
    zi_in_mem in{ view };
    std::vector<zi_tables> S(1);
    S[0].kind = 0;
    zi_out_linear<> o{ zi_view<uint8_t>{ out, cap }, 0, 0, 1, {} };
    const zi_result R = zi_run(in, view, 0, o, S[0], ZI_RUN_STREAM, 0, 0, 1);
    if (R.err) return R.err == ZI_E_SPACE ? ZI_ITEM_NOSPACE : ZI_ITEM_DATA;
    if (R.end > view.n || view.n - R.end != tlen(format)) return ZI_ITEM_DATA;
    std::vector<zi_sum> sum(1);
    sum[0].init(format);
    sum[0].add(zi_view<const uint8_t>{ out, R.out }, 0, R.out);
    if (!sum[0].trailer_ok(zi_view<const uint8_t>{ view.p + R.end, tlen(format) }, R.out)) return ZI_ITEM_DATA;
    *out_len = R.out;
    return ZI_ITEM_OK;
}

}  // namespace

// the builder, row for row what zz_points_index_host gives; *entries is set for every valid stream
extern "C" int zpt_build(const uint8_t* src, uint64_t n, int format, uint64_t spacing, uint64_t* rows, uint64_t max_entries,
                         uint64_t* entries, uint64_t* out_len)
{
    *entries = 0; *out_len = 0;
    std::vector<uint8_t> copy(src, src + n);                  // exactly the stream's bytes: the checker sees overreads
    row_sink sink;
    std::vector<uint8_t> ring(ZI_RING);
    std::vector<zi_tables> S(1);
    std::vector<zi_sum> sum(1);
    const int rc = zi_points_build(copy.data(), n, format, spacing, sink, ring.data(), S[0], sum[0], out_len);
    if (rc) return rc;
    *entries = sink.rows.size() / 2;
    if (*entries > max_entries) return ZI_ITEM_NOSPACE;
    memcpy(rows, sink.rows.data(), sink.rows.size() * 8);
    return ZI_ITEM_OK;
}

// The whole call. status: 0 ok, -2 no space, -5 preset dictionary, -6 data (the ABI's codes); -100: the lanes disagree.
// stats[0] pending bytes, [1] rounds (the most of any batch), [2] batches, [3] segments whose run refused (every segment of the
// call is run, also behind a refusal), [4] 1: zi_points_check (or the trailer's place) refused the index, [5] the path: 4 points,
// 3 serial, [6] 1: the points path decoded everything but the checksum refused it.
extern "C" int zpt_decode(const uint8_t* src, uint64_t n, int format, const uint64_t* rows, uint64_t entries, uint8_t* out, uint64_t cap,
                          uint64_t batch_limit, uint32_t lanes, uint64_t* out_len, uint64_t* stats)
{
    *out_len = 0;
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES) return -100;
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return ZI_ITEM_UNSUPPORTED;
    if (hl < 0 || n - (uint64_t)hl < tlen(format)) return ZI_ITEM_DATA;
    const uint64_t sn = n - (uint64_t)hl - tlen(format);
    std::vector<uint8_t> defl(src + hl, src + hl + sn);       // exactly the DEFLATE bytes
    bool done = false;
    uint64_t total = 0;
    if (entries >= 2 && zi_points_check(rows, entries, sn, cap, batch_limit) && (rows[2 * (entries - 1)] + 7) / 8 == sn) {
        const uint64_t nseg_total = entries - 1;
        std::vector<zi_tables> S(1);
        bool refused = false;
        for (uint64_t k0 = 0, k1; k0 < nseg_total; k0 = k1) {
            k1 = zi_points_batches(rows, entries, k0, batch_limit, 1u << 20);
            ++stats[2];
            const uint64_t base = rows[2 * k0 + 1], nbytes = rows[2 * k1 + 1] - base;
            const uint64_t tiles = (nbytes + ZI_POINTS_TILE - 1) / ZI_POINTS_TILE, words = tiles * (ZI_POINTS_TILE / 32);
            std::vector<uint32_t> st(nbytes + 1, 0), pend(words + 1, 0), pcnt(tiles + 1, 0);
            uint64_t npend_lanes = 0;
            for (uint64_t k = k0; k < k1; ++k) {              // phase 1
                g_seg.view = zi_view<const uint8_t>{ defl.data(), sn };
                g_seg.b0 = rows[2 * k]; g_seg.o0 = rows[2 * k + 1]; g_seg.b1 = rows[2 * k + 2]; g_seg.o1 = rows[2 * k + 3];
                g_seg.last = k + 1 == nseg_total;
                g_seg.dst = out; g_seg.base = base; g_seg.nbytes = nbytes;
                g_seg.st = st.data(); g_seg.pend = pend.data(); g_seg.words = words; g_seg.S = &S[0];
                if (!run_segment(lanes)) return -100;
                if (g_seg.res[0].err) { ++stats[3]; refused = true; continue; }
                if (g_seg.end_bit[0] != g_seg.b1 || g_seg.res[0].out != g_seg.o1 - g_seg.o0) return -100;   // (ZI_RUN_POINT's own promise)
                for (uint32_t l = 0; l < lanes; ++l) npend_lanes += g_seg.npend[l];
            }
            if (refused) continue;                            // the device stops here; the harness still runs every segment
            uint64_t batch_pend = 0;
            for (uint64_t t = 0; t < tiles; ++t) {            // the tile counts
                uint32_t c = 0;
                for (uint32_t w = 0; w < ZI_POINTS_TILE / 32; ++w) c += zi_popc32(pend[t * (ZI_POINTS_TILE / 32) + w]);
                pcnt[t] = c; batch_pend += c;
            }
            if (batch_pend != npend_lanes) return -100;       // the bitmap holds what the lanes counted
            stats[0] += batch_pend;
            if (!batch_pend) continue;
            // the rounds: k_inflate_resolve's rule over tiles of ZI_POINTS_TILE bytes, a round reading what the round before left
            auto pending = [&](uint64_t x) { return pcnt[x / ZI_POINTS_TILE] && ((pend[x >> 5] >> (x & 31)) & 1u); };
            std::vector<uint64_t> open, still;                // the bytes not final yet
            for (uint64_t x = 0; x < nbytes; ++x) if (pending(x)) open.push_back(x);
            std::vector<uint32_t> adopted;                    // this round's new pointers of `still`, stored when the round is over
            std::vector<uint8_t> done_round(nbytes, 0);
            for (uint32_t round = 1;; ++round) {
                still.clear(); adopted.clear();
                for (const uint64_t x : open) {
                    const int64_t y = (int64_t)(st[x] & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
                    if ((int64_t)base + y < 0 || y >= (int64_t)x) return -100;            // in front of the stream, or not in front of x
                    if (y < 0 || !pending((uint64_t)y) || (done_round[(uint64_t)y] && done_round[(uint64_t)y] < round)) {
                        out[base + x] = out[(int64_t)base + y]; done_round[x] = (uint8_t)round;
                    } else { still.push_back(x); adopted.push_back(st[(uint64_t)y]); }
                }
                for (uint64_t i = 0; i < still.size(); ++i) st[still[i]] = adopted[i];
                open.swap(still);
                if (open.empty()) { if (round > stats[1]) stats[1] = round; break; }
                if (round > ZI_ROUND_EXTERNAL - 1) return -100;
            }
        }
        if (!refused) {
            total = rows[2 * nseg_total + 1];
            std::vector<zi_sum> sum(1);
            sum[0].init(format);
            sum[0].add(zi_view<const uint8_t>{ out, total }, 0, total);
            done = sum[0].trailer_ok(zi_view<const uint8_t>{ src + n - tlen(format), tlen(format) }, total);
            if (!done) stats[6] = 1;
        }
    } else stats[4] = 1;
    if (done) { stats[5] = 4; *out_len = total; return ZI_ITEM_OK; }
    stats[0] = stats[1] = 0;
    stats[5] = 3;
    return serial(src, n, format, out, cap, out_len);
}

// every segment decoded ALONE, with nothing but the true 32 KiB in front of it: its bytes are its slice of `data`
extern "C" uint64_t zpt_segments_alone(const uint8_t* src, uint64_t n, int format, const uint64_t* rows, uint64_t entries,
                                       const uint8_t* data, uint64_t data_len)
{
    const int64_t hl = zi_header(format, src, n);
    if (hl < 0 || entries < 2 || n - (uint64_t)hl < tlen(format)) return ~0ull;
    const uint64_t sn = n - (uint64_t)hl - tlen(format);
    std::vector<uint8_t> defl(src + hl, src + hl + sn);
    const zi_view<const uint8_t> view{ defl.data(), sn };
    std::vector<zi_tables> S(1);
    uint64_t bad = 0;
    for (uint64_t k = 0; k + 1 < entries; ++k) {
        const uint64_t b0 = rows[2 * k], o0 = rows[2 * k + 1], b1 = rows[2 * k + 2], o1 = rows[2 * k + 3];
        if (o1 < o0 || o1 > data_len) { ++bad; continue; }
        const uint64_t front = o0 < ZI_BIAS ? o0 : ZI_BIAS;
        std::vector<uint8_t> buf(data + o0 - front, data + o0);
        buf.resize(front + (o1 - o0), 0xEE);
        zi_in_mem in{ view };
        zi_out_linear<> o{ zi_view<uint8_t>{ buf.data(), buf.size() }, front, 0, 1, {} };
        zi_pt_segment pt{ (uint32_t)(b0 & 7), b1, k + 2 == entries, 0 };
        S[0].kind = 0;
        const zi_result R = zi_run(in, view, b0 >> 3, o, S[0], ZI_RUN_POINT, front + (o1 - o0), 0, 1, pt);
        if (R.err || (o1 > o0 && memcmp(buf.data() + front, data + o0, o1 - o0) != 0)) ++bad;
    }
    return bad;
}
