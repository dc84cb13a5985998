// inflate_points_ranges_harness.cpp -- CPU harness of zz_points_windows_host and zz_decode_points_ranges_device
// (zzflate_amd/csrc/zz_inflate_core.h: zi_points_windows_build, zi_out_window, zi_pr_*, and the zi_mr_* rules called with a point
// index): the bounds-checked host restatement of the builder pass and of the whole call -- argument checks, index check, front
// (header, last bit, the fold of the sums in the device's own order: 1024 runs of consecutive entries, then a tree), plan,
// differences, touched scan, waves, per touched segment ZI_RUN_POINT onto a stage against its window slot, its sum, F, cut,
// chunked copy, verdict -- with the very functions the kernels of zz_inflate_points_ranges.h and zz_inflate_members_ranges.h call.
// tests/points_ranges_cases.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every access of the core and of this
// file's tables goes through a checked view; out of range aborts the process), once with the product's ZZ_MR_STAGE and once with a
// stage of a few hundred bytes, so that waves and big segments occur on small inputs.
//
//   zpr_windows(src, n, format, rows, entries, windows, sums) -> status
//   zpr_reads(src, n, format, rows, entries, windows, sums, nranges, firsts, nbytes, dsts, caps, out_lens, status, lanes,
//             &segments_decoded, &waves, win_copied) -> the call's code; win_copied (may be null): per segment, bytes copied from its window
//   zpr_fold(format, sums, lens, n, &value) -> 1: every entry is one its length can have; value = the public checksum of the whole
//   zpr_stage() -> ZZ_MR_STAGE of this build
//
// Simulated lanes (lanes = 2..64), as in inflate_points_harness.cpp: every lane is a coroutine running the segment's zi_run with
// its own lane number over the SAME tables and stage slot; a lane runs alone until it depends on what other lanes wrote --
// ZI_LANES_SYNC() in the table builder, the out policy's fence in front of a copy -- and there the next lane runs, round robin.
#define HARNESS_NAME "inflate_points_ranges_harness"
#include "harness_reads.h"

using namespace zz;

namespace {

constexpr uint32_t FRONT_THREADS = 1024;

// one segment's run, as k_inflate_segments_win sets it up
struct seg_call {
    zi_view<const uint8_t> view;               // the DEFLATE bytes (no trailer)
    zi_pr_slot d;
    zi_view<uint8_t> slot;                     // its slot on the stage
    zi_view<const uint8_t> win;                // its window slot
    zi_tables* S;
    zi_result res[MAX_LANES]; uint64_t end_bit[MAX_LANES]; uint64_t from_win[MAX_LANES];
};
seg_call g_seg;

void lane_main(int lane)
{
    seg_call& c = g_seg;
    zi_in_mem in{ c.view };
    zi_out_window<host_fence> o{ c.slot, c.win, c.d.o0, 0, 0, (uint32_t)lane, g_nl, {} };
    zi_pt_segment pt{ (uint32_t)(c.d.b0 & 7), c.d.b1, c.d.last, 0 };
    c.res[lane] = zi_run(in, c.view, c.d.b0 >> 3, o, *c.S, ZI_RUN_POINT, c.d.room, (uint32_t)lane, g_nl, pt);
    c.end_bit[lane] = pt.end_bit;
    c.from_win[lane] = o.from_win;
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

// k_pr_front's fold: thread t joins the entries [t * per, (t + 1) * per), a tree joins the threads in order
bool fold(int kind, const zi_view<const uint32_t>& sums, const std::vector<uint64_t>& lens, zi_pr_part* all)
{
    const uint64_t segments = lens.size();
    const uint64_t per = (segments + FRONT_THREADS - 1) / FRONT_THREADS;
    std::vector<zi_pr_part> part(FRONT_THREADS, zi_pr_part{ 0, 0 });
    bool ok = true;
    for (uint64_t t = 0; t < FRONT_THREADS; ++t) {
        const uint64_t j0 = t * per < segments ? t * per : segments, j1 = j0 + per < segments ? j0 + per : segments;
        for (uint64_t j = j0; j < j1; ++j) {
            zi_pr_part p;
            if (!zi_pr_entry_part(kind, sums[j], lens[j], &p)) ok = false;
            part[t] = zi_pr_join(kind, part[t], p);
        }
    }
    for (uint32_t s = 1; s < FRONT_THREADS; s <<= 1)
        for (uint32_t t = 0; t < FRONT_THREADS; t += 2 * s) part.at(t) = zi_pr_join(kind, part.at(t), part.at(t + s));
    *all = part[0];
    return ok;
}

}  // namespace

extern "C" uint64_t zpr_stage(void) { return ZZ_MR_STAGE; }

extern "C" int zpr_fold(int format, const uint32_t* sums, const uint64_t* lens, uint64_t n, uint32_t* value)
{
    const int kind = zi_sidecar_kind(format);
    const std::vector<uint32_t> s(sums, sums + n);
    const std::vector<uint64_t> l(lens, lens + n);
    zi_pr_part all{ 0, 0 };
    const bool ok = fold(kind, view_of(s), l, &all);
    *value = kind == ZI_CKS_ADLER ? adler_combine(1u, all.v, all.len) : all.v;
    return ok ? 1 : 0;
}

// the builder, what zz_points_windows_host gives: the ABI's codes (0, -4, -5, -6)
extern "C" int zpr_windows(const uint8_t* src, uint64_t n, int format, const uint64_t* rows, uint64_t entries, uint8_t* windows, uint32_t* sums)
{
    if (!src || !rows || !windows || !sums || entries < 2 || format < 0 || format > 2) return ZI_RV_ARG;
    const std::vector<uint8_t> copy(src, src + n);            // exactly the stream's bytes: the checker sees overreads
    const std::vector<uint64_t> r(rows, rows + 2 * entries);
    std::vector<uint8_t> ring(ZI_RING);
    std::vector<zi_tables> S(1);
    std::vector<zi_sum> sum(1);
    return zi_points_windows_build(copy.data(), n, format, r.data(), entries, windows, sums, ring.data(), S[0], sum[0]);
}

// The whole call. The ABI's codes: 0 ok, -2 no space, -4 argument, -5 unsupported, -6 data; -100: the lanes disagree.
extern "C" int zpr_reads(const uint8_t* src_in, uint64_t src_len, int format, const uint64_t* rows, uint64_t entries,
                         const uint8_t* windows_in, const uint32_t* sums_in, uint64_t nranges,
                         const uint64_t* firsts, const uint64_t* nbytes, uint8_t* const* dsts, const uint64_t* caps,
                         uint64_t* out_lens, int32_t* status, uint32_t lanes, uint64_t* segments_decoded, uint32_t* waves, uint64_t* win_copied)
{
    *segments_decoded = 0; *waves = 0;
    if (lanes < 1 || lanes > MAX_LANES) return -100;
    if (!src_in || !rows || !windows_in || !sums_in || !firsts || !nbytes || !dsts || !caps || !out_lens) return ZI_RV_ARG;
    if (entries < 2 || entries - 1 > 0x7fffffffull || nranges > 0x7fffffffull || format < 0 || format > 2) return ZI_RV_ARG;
    if (nranges == 0) return ZI_RV_OK;
    const uint64_t segments = entries - 1;
    const std::vector<uint8_t> src(src_in, src_in + src_len);                     // exactly the stream's bytes
    const std::vector<uint64_t> idxv(rows, rows + 2 * entries);                   // exactly the index's words
    const std::vector<uint8_t> windows(windows_in, windows_in + segments * ZI_PR_WINDOW);
    const std::vector<uint32_t> sums(sums_in, sums_in + segments);
    const zi_view<const uint64_t> idx = view_of(idxv);
    const int kind = zi_sidecar_kind(format);
    if (win_copied) for (uint64_t j = 0; j < segments; ++j) win_copied[j] = 0;

    // check (the last bit bounded by eight times the source) and front
    bool index_bad = false;
    for (uint64_t j = 0; j < entries; ++j) if (zi_mr_entry_bad(idx, entries, j, src_len > (~0ull >> 3) ? ~0ull : 8 * src_len)) index_bad = true;
    const int64_t hl = zi_header(format, src.data(), src_len);
    uint64_t sn = 0;
    const uint64_t tl = format == 0 ? 4 : format == 1 ? 8 : 0;
    {
        std::vector<uint64_t> lens(segments);
        for (uint64_t j = 0; j < segments; ++j) lens[j] = zi_mr_u(idx, j + 1) - zi_mr_u(idx, j);
        zi_pr_part all{ 0, 0 };
        const bool entries_ok = fold(kind, view_of(sums), lens, &all);
        const bool ok = zi_pr_deflate_len(format, src_len, hl, &sn) && zi_pr_ends_ok(zi_mr_c(idx, 0), zi_mr_c(idx, segments), sn) && entries_ok &&
                        zi_pr_trailer_ok(format, src.data() + (src_len - tl), zi_pr_part{ all.v, zi_mr_u(idx, segments) });
        if (!ok) index_bad = true;
    }
    if (index_bad) {
        reads_all_fail(nranges, out_lens, status);
        return hl == -2 ? ZI_RV_UNSUPPORTED : ZI_RV_DATA;
    }
    const std::vector<uint8_t> defl(src.begin() + hl, src.begin() + hl + sn);     // exactly the DEFLATE bytes
    // the rest is harness_reads.h's; per touched segment: its rows, ZI_RUN_POINT onto its slot against its window slot, its sum
    std::vector<zi_tables> tables(1);
    const host_lanes one{ 0 };                                                    // zi_adler_lanes / zi_crc_lanes with one lane
    return reads_through_index(idx, entries, nranges, firsts, nbytes, dsts, caps, out_lens, status, waves,
        [&](const zi_mr_tables& tab, uint64_t t, uint64_t t0, std::vector<uint8_t>& stage, unit_result* u) {
            const zi_pr_slot d = zi_pr_desc(tab, entries, t, t0);
            *u = unit_result{ ZI_ITEM_DATA, ~0ull, d.room };
            if (d.skip) return true;
            const zi_view<uint8_t> whole{ stage.data(), stage.size() };
            if (d.room) (void)whole[d.stage_off + d.room - 1];                   // the slot lies inside the stage
            (void)view_of(windows)[d.seg * ZI_PR_WINDOW + ZI_PR_WINDOW - 1];     // the window slot lies inside the windows
            g_seg.view = view_of(defl);
            g_seg.d = d;
            g_seg.slot = zi_view<uint8_t>{ stage.data() + d.stage_off, d.room };
            g_seg.win = zi_view<const uint8_t>{ windows.data() + d.seg * ZI_PR_WINDOW, ZI_PR_WINDOW };
            g_seg.S = &tables[0];
            if (!run_segment(lanes)) return false;
            const zi_result& R = g_seg.res[0];
            uint32_t sum = 0;
            if (!R.err) {
                if (g_seg.end_bit[0] != d.b1 || R.out != d.room) return false;   // (ZI_RUN_POINT's own promise)
                const zi_view<const uint8_t> slot{ stage.data() + d.stage_off, d.room };
                sum = kind == ZI_CKS_ADLER ? zi_adler_lanes(one, slot, d.room, 0, 1) : zi_crc_lanes(one, slot, d.room, 0, 1);
            }
            u->status = zi_pr_segment_status(R.err, R.out, d.room, sum, view_of(sums)[d.seg]);
            if (u->status == ZI_ITEM_OK) u->out = R.out;
            if (win_copied) for (uint32_t l = 0; l < lanes; ++l) win_copied[d.seg] += g_seg.from_win[l];
            ++*segments_decoded;
            return true;
        });
}
