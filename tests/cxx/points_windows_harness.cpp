// points_windows_harness.cpp -- CPU harness of zz_points_windows_device and zz_points_thin (zzflate_amd/csrc/zz_inflate_core.h:
// zi_pw_*, zi_points_superset, zi_points_thin, and ZI_RUN_POINT, zi_out_segment, zi_points_check, zi_points_batches, zi_pr_*): the
// bounds-checked host restatement of the whole call -- argument checks, container, index checks, the batches planned over the
// sidecar's rows, per unit the decode with the finer rows (phase 1 per segment as k_inflate_segments sets it up, the tile counts,
// the rounds) onto a stage of 32 KiB carry + the batch addressed by absolute position, the cut (k_points_windows_cut: slots, sums,
// the next batch's first slot as the carry), the pieces of a sidecar segment longer than the stage, the fold and the trailer's
// verdict. tests/points_windows_cases.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every access of the core
// and of the stage goes through a checked view; out of range aborts the process) and calls it through ctypes.
//
//   zpw_build(src, n, format, rows, entries, fine, fine_entries, windows, sums, dst, cap, stage_bytes, lanes, stats) -> status
//        the ABI's codes: 0 ok, -2 no space, -4 argument, -5 unsupported, -6 data; -100: the harness contradicts itself.
//        stats[0] decode batches, [1] pending bytes, [2] rounds (the most of any batch), [3] units whose base lies below 32768 (the
//        first one not counted), [4] slots that took bytes from both the carry and the batch, [5] sidecar segments cut in pieces
//   zpw_thin(rows, entries, spacing, out, max_entries, &out_entries) -> status
//   zpw_superset(rows, entries, fine, fine_entries) -> 1: accepted
//
// Simulated lanes (lanes = 2..64), as in inflate_points_harness.cpp: every lane is a coroutine over the SAME tables, stage, bitmap
// and pointers; a lane runs alone until it depends on what other lanes wrote, and there the next lane runs, round robin.
#define HARNESS_NAME "points_windows_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

constexpr uint64_t BATCH_BYTES = 64ull << 20;                // ZZ_INF_BATCH_BYTES
constexpr uint64_t BATCH_SEGMENTS = 1ull << 20;              // ZZ_PT_BATCH_SEGMENTS

// one segment's phase 1, as k_inflate_segments sets it up; `out` is the segment's place on the stage
struct seg_call {
    zi_view<const uint8_t> view;               // the DEFLATE bytes (no trailer)
    uint64_t b0, o0, b1, o1; bool last;
    zi_view<uint8_t> out; uint64_t base, nbytes;
    uint32_t* st; uint32_t* pend; uint64_t words;
    zi_tables* S;
    zi_result res[MAX_LANES]; uint64_t end_bit[MAX_LANES]; uint32_t npend[MAX_LANES];
};
seg_call g_seg;

void seg_lane(int lane)
{
    seg_call& c = g_seg;
    zi_in_mem in{ c.view };
    zi_out_segment<host_fence, zi_bits_plain> o{ c.out, zi_view<uint32_t>{ c.pend, c.words }, zi_view<uint32_t>{ c.st, c.nbytes }, c.o0,
                                                 c.o0 - c.base, 0, 0, false, (uint32_t)lane, g_nl, {}, {} };
    zi_pt_segment pt{ (uint32_t)(c.b0 & 7), c.b1, c.last, 0 };
    c.res[lane] = zi_run(in, c.view, c.b0 >> 3, o, *c.S, ZI_RUN_POINT, c.o1 - c.o0, (uint32_t)lane, g_nl, pt);
    c.end_bit[lane] = pt.end_bit;
    c.npend[lane] = o.npend;
}

bool run_segment(uint32_t lanes)
{
    memset(g_seg.S, 0xA5, sizeof *g_seg.S);                   // nothing may rely on what the tables held
    g_seg.S->kind = 0;
    if (!run_lanes(lanes, seg_lane)) return false;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_seg.res[l].err != g_seg.res[0].err || g_seg.res[l].out != g_seg.res[0].out || g_seg.res[l].final != g_seg.res[0].final ||
            g_seg.end_bit[l] != g_seg.end_bit[0]) return false;
    return true;
}

// one item of k_points_windows_cut
struct cut_call {
    zi_view<const uint8_t> buf; int64_t org; int kind;
    uint64_t o0, o1; bool sum_it;
    zi_view<uint8_t> slot;
    uint32_t sum[MAX_LANES];
};
cut_call g_cut;

void cut_lane(int lane)
{
    cut_call& c = g_cut;
    host_lanes w{ (uint32_t)lane };
    zi_pw_slot_copy(c.buf, c.slot, zi_pw_slot_place(c.o0, c.org), (uint32_t)lane, g_nl);
    c.sum[lane] = c.sum_it ? zi_pw_segment_sum(w, c.kind, c.buf, c.org, c.o0, c.o1, (uint32_t)lane, g_nl) : 0u;
}

bool run_cut(uint32_t lanes)
{
    if (!run_lanes(lanes, cut_lane)) return false;
    for (uint32_t l = 1; l < lanes; ++l) if (g_cut.sum[l] != g_cut.sum[0]) return false;
    return true;
}

uint64_t tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }

// the call's state: what pw_run_unit of zz_api.hip works on
struct call {
    zi_view<const uint8_t> defl;
    const uint64_t* dec; uint64_t dec_entries;
    uint8_t* dst;                               // null: the stage
    std::vector<uint8_t> stage;
    uint64_t stage_bytes; int kind; uint32_t lanes;
    std::vector<zi_tables> S;
    uint64_t* stats;
    bool first_unit;
};

struct unit {
    uint64_t g0, g1;
    const uint64_t* cut_rows; uint32_t ncut;
    uint8_t* win_dst; uint32_t* sum_dst; uint8_t* tail_dst;
};

// 0, ZI_ITEM_DATA, or -100
int run_unit(call& C, const unit& U)
{
    const uint64_t base = C.dec[2 * U.g0 + 1], end = C.dec[2 * U.g1 + 1];
    const int64_t org = zi_pw_org(base, C.dst != nullptr);
    const zi_view<uint8_t> buf{ C.dst ? C.dst : C.stage.data(), C.dst ? end : ZI_PR_WINDOW + (end - base) };
    if (!C.dst && buf.n > C.stage.size()) return -100;       // the stage holds the unit
    if (!C.first_unit && base < ZI_PR_WINDOW) ++C.stats[3];
    C.first_unit = false;
    auto at = [&](int64_t abs) -> uint8_t& { return buf[(uint64_t)(abs - org)]; };
    for (uint64_t h0 = U.g0, h1; h0 < U.g1; h0 = h1) {
        h1 = zi_points_batches(C.dec, U.g1 + 1, h0, C.stage_bytes, BATCH_SEGMENTS);
        ++C.stats[0];
        const uint64_t sb = C.dec[2 * h0 + 1], nbytes = C.dec[2 * h1 + 1] - sb;
        const uint64_t tiles = (nbytes + ZI_POINTS_TILE - 1) / ZI_POINTS_TILE, words = tiles * (ZI_POINTS_TILE / 32);
        std::vector<uint32_t> st(nbytes + 1, 0), pend(words + 1, 0), pcnt(tiles + 1, 0);
        uint64_t npend_lanes = 0;
        for (uint64_t k = h0; k < h1; ++k) {                  // phase 1
            g_seg.view = C.defl;
            g_seg.b0 = C.dec[2 * k]; g_seg.o0 = C.dec[2 * k + 1]; g_seg.b1 = C.dec[2 * k + 2]; g_seg.o1 = C.dec[2 * k + 3];
            g_seg.last = k + 2 == C.dec_entries;
            if (g_seg.o1 > g_seg.o0) { (void)at((int64_t)g_seg.o0); (void)at((int64_t)g_seg.o1 - 1); }    // the segment lies on the stage
            g_seg.out = zi_view<uint8_t>{ buf.p + (uint64_t)((int64_t)g_seg.o0 - org), g_seg.o1 - g_seg.o0 };
            g_seg.base = sb; g_seg.nbytes = nbytes;
            g_seg.st = st.data(); g_seg.pend = pend.data(); g_seg.words = words; g_seg.S = &C.S[0];
            if (!run_segment(C.lanes)) return -100;
            if (g_seg.res[0].err) return ZI_ITEM_DATA;
            if (g_seg.end_bit[0] != g_seg.b1 || g_seg.res[0].out != g_seg.o1 - g_seg.o0) return -100;   // (ZI_RUN_POINT's own promise)
            for (uint32_t l = 0; l < C.lanes; ++l) npend_lanes += g_seg.npend[l];
        }
        uint64_t batch_pend = 0;
        for (uint64_t t = 0; t < tiles; ++t) {                // the tile counts
            uint32_t n = 0;
            for (uint32_t w = 0; w < ZI_POINTS_TILE / 32; ++w) n += zi_popc32(pend[t * (ZI_POINTS_TILE / 32) + w]);
            pcnt[t] = n; batch_pend += n;
        }
        if (batch_pend != npend_lanes) return -100;
        C.stats[1] += batch_pend;
        if (!batch_pend) continue;
        // the rounds: k_inflate_resolve's rule over tiles of ZI_POINTS_TILE bytes, a round reading what the round before left; a
        // pointer below the batch base is a byte of an earlier batch on the stage -- at most ZI_BIAS down, inside the carry
        auto pending = [&](uint64_t x) { return pcnt[x / ZI_POINTS_TILE] && ((pend[x >> 5] >> (x & 31)) & 1u); };
        std::vector<uint64_t> open, still;
        for (uint64_t x = 0; x < nbytes; ++x) if (pending(x)) open.push_back(x);
        std::vector<uint32_t> adopted;
        std::vector<uint8_t> done_round(nbytes, 0);
        for (uint32_t round = 1;; ++round) {
            still.clear(); adopted.clear();
            for (const uint64_t x : open) {
                const int64_t y = (int64_t)(st[x] & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
                if ((int64_t)sb + y < 0 || y >= (int64_t)x) return -100;                  // in front of the stream, or not in front of x
                if (y < 0 || !pending((uint64_t)y) || (done_round[(uint64_t)y] && done_round[(uint64_t)y] < round)) {
                    at((int64_t)(sb + x)) = at((int64_t)sb + y); done_round[x] = (uint8_t)round;
                } else { still.push_back(x); adopted.push_back(st[(uint64_t)y]); }
            }
            for (uint64_t i = 0; i < still.size(); ++i) st[still[i]] = adopted[i];
            open.swap(still);
            if (open.empty()) { if (round > C.stats[2]) C.stats[2] = round; break; }
            if (round > ZI_ROUND_EXTERNAL - 1) return -100;
        }
    }
    // the cut
    const uint64_t items = (uint64_t)U.ncut + (U.tail_dst ? 1 : 0);
    for (uint64_t i = 0; i < items; ++i) {
        g_cut.buf = zi_view<const uint8_t>{ buf.p, buf.n }; g_cut.org = org; g_cut.kind = C.kind;
        g_cut.o0 = U.cut_rows[2 * i + 1]; g_cut.sum_it = i < U.ncut; g_cut.o1 = g_cut.sum_it ? U.cut_rows[2 * i + 3] : 0;
        g_cut.slot = zi_view<uint8_t>{ i < U.ncut ? U.win_dst + i * ZI_PR_WINDOW : U.tail_dst, ZI_PR_WINDOW };
        if (!run_cut(C.lanes)) return -100;
        if (i < U.ncut) U.sum_dst[i] = g_cut.sum[0];
        if (!C.dst && base > 0 && g_cut.o0 > base && g_cut.o0 - base < ZI_PR_WINDOW) ++C.stats[4];   // carry and batch both
    }
    if (U.tail_dst && !C.dst) memcpy(C.stage.data(), U.tail_dst, ZI_PR_WINDOW);     // the next carry
    return 0;
}

}  // namespace

extern "C" int zpw_thin(const uint64_t* rows, uint64_t entries, uint64_t spacing, uint64_t* out, uint64_t max_entries, uint64_t* out_entries)
{
    if (!rows || !out_entries) return ZI_RV_ARG;
    *out_entries = 0;
    if (entries < 2 || spacing == 0) return ZI_RV_ARG;
    const std::vector<uint64_t> r(rows, rows + 2 * entries);
    *out_entries = zi_points_thin(r.data(), entries, spacing, nullptr, 0);
    if (!out || max_entries < *out_entries) return ZI_ITEM_NOSPACE;
    std::vector<uint64_t> o(2 * *out_entries);
    zi_points_thin(r.data(), entries, spacing, o.data(), *out_entries);
    memcpy(out, o.data(), o.size() * 8);
    return ZI_ITEM_OK;
}

extern "C" int zpw_superset(const uint64_t* rows, uint64_t entries, const uint64_t* fine, uint64_t fine_entries)
{
    const std::vector<uint64_t> r(rows, rows + 2 * entries), f(fine, fine + 2 * fine_entries);
    return zi_points_superset(r.data(), entries, f.data(), fine_entries) ? 1 : 0;
}

extern "C" int zpw_build(const uint8_t* src, uint64_t n, int format, const uint64_t* rows_in, uint64_t entries, const uint64_t* fine_in,
                         uint64_t fine_entries, uint8_t* windows, uint32_t* sums, uint8_t* dst, uint64_t cap, uint64_t stage_bytes,
                         uint32_t lanes, uint64_t* stats)
{
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES) return -100;
    if (!src || !rows_in || !windows || !sums) return ZI_RV_ARG;
    if (entries < 2 || entries - 1 > 0x7fffffffull || format < 0 || format > 2 || stage_bytes > BATCH_BYTES || (!dst && cap)) return ZI_RV_ARG;
    const std::vector<uint64_t> rowsv(rows_in, rows_in + 2 * entries);            // exactly the rows' words
    const std::vector<uint64_t> finev(fine_in ? fine_in : rows_in, (fine_in ? fine_in : rows_in) + 2 * (fine_in ? fine_entries : 0));
    const uint64_t* const points = rowsv.data();
    if (fine_in && !zi_points_superset(points, entries, finev.data(), fine_entries)) return ZI_RV_ARG;
    const uint64_t segments = entries - 1, L = points[2 * segments + 1];
    if (dst && cap < L) return ZI_ITEM_NOSPACE;
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return ZI_ITEM_UNSUPPORTED;
    if (hl < 0 || n < (uint64_t)hl + tlen(format)) return ZI_ITEM_DATA;
    const uint64_t sn = n - (uint64_t)hl - tlen(format);
    const std::vector<uint8_t> defl(src + hl, src + hl + sn);                     // exactly the DEFLATE bytes
    const uint64_t stage = stage_bytes ? stage_bytes : BATCH_BYTES;
    const uint64_t* const dec = fine_in ? finev.data() : points;
    const uint64_t dec_entries = fine_in ? fine_entries : entries;
    if (!zi_points_check(points, entries, sn, ~0ull, ~0ull) || !zi_points_check(dec, dec_entries, sn, ~0ull, ~0ull) ||
        (points[2 * segments] + 7) / 8 != sn) return ZI_ITEM_DATA;
    if (!zi_points_check(dec, dec_entries, sn, ~0ull, stage)) return ZI_ITEM_UNSUPPORTED;
    const uint64_t most = L < stage ? (L ? L : 1) : stage;
    call C{ view_of(defl), dec, dec_entries, dst, std::vector<uint8_t>(dst ? 0 : ZI_PR_WINDOW + most, 0xEE), stage, zi_sidecar_kind(format),
            lanes, std::vector<zi_tables>(1), stats, true };
    std::vector<uint8_t> spare(2 * ZI_PR_WINDOW, 0xEE);
    zi_pr_part all{ 0, 0 };
    uint64_t f0 = 0;
    for (uint64_t k0 = 0, k1; k0 < segments; k0 = k1) {
        k1 = zi_points_batches(points, entries, k0, stage, BATCH_SEGMENTS);
        uint64_t f1 = f0 + (k1 - k0);
        if (fine_in) for (f1 = f0 + 1; f1 + 1 < fine_entries && dec[2 * f1] != points[2 * k1]; ++f1) {}
        uint8_t* const tail = k1 < segments ? windows + k1 * ZI_PR_WINDOW : nullptr;
        if (points[2 * k1 + 1] - points[2 * k0 + 1] <= stage) {
            const unit U{ f0, f1, points + 2 * k0, (uint32_t)(k1 - k0), windows + k0 * ZI_PR_WINDOW, sums + k0, tail };
            if (const int rc = run_unit(C, U)) return rc;
            for (uint64_t k = k0; k < k1; ++k) {
                zi_pr_part p;
                if (!zi_pr_entry_part(C.kind, sums[k], points[2 * k + 3] - points[2 * k + 1], &p)) return -100;
                all = zi_pr_join(C.kind, all, p);
            }
        } else {
            ++stats[5];
            zi_pr_part seg{ 0, 0 };
            for (uint64_t g0 = f0, g1; g0 < f1; g0 = g1) {
                g1 = zi_points_batches(dec, f1 + 1, g0, stage, BATCH_SEGMENTS);
                const uint64_t piece_rows[4] = { dec[2 * g0], dec[2 * g0 + 1], dec[2 * g1], dec[2 * g1 + 1] };
                uint32_t v = 0;
                const unit U{ g0, g1, piece_rows, 1, g0 == f0 ? windows + k0 * ZI_PR_WINDOW : spare.data(), &v,
                              g1 == f1 ? tail : spare.data() + ZI_PR_WINDOW };
                if (const int rc = run_unit(C, U)) return rc;
                zi_pr_part p;
                if (!zi_pr_entry_part(C.kind, v, piece_rows[3] - piece_rows[1], &p)) return -100;
                seg = zi_pr_join(C.kind, seg, p);
            }
            sums[k0] = zi_pr_public(C.kind, seg);
            all = zi_pr_join(C.kind, all, seg);
        }
        f0 = f1;
    }
    if (all.len != L || !zi_pr_trailer_ok(format, src + n - tlen(format), all)) return ZI_ITEM_DATA;
    return ZI_ITEM_OK;
}
