// points_find_harness.cpp -- CPU harness of the point index found in parallel (zzflate_amd/csrc/zz_inflate_core.h: zi_find_prefilter,
// zi_find_header, zi_out_count, zi_pt_reach / ZI_RUN_REACH, zi_find_link, zi_find_rows), the host restatement of
// zz_points_index_device: the finder chunk by chunk (k_points_find), the reach jobs of a round (k_points_reach), the links, the
// repair rounds, the rows and the trailer's place. tests/test_points_find_cpu.py builds it with g++ -fsanitize=undefined
// -DZZ_INFLATE_CHECKED (every buffer access of the core checked; out of range aborts the process) and calls it through ctypes;
// tests/cxx/points_find_main.cpp is the same code behind a main() for a stand-alone sanitizer build.
//
//   zpf_index(src, n, format, chunk, spacing, limit_bytes, lanes, rows, max_entries, &entries, &out_len, stats) -> status
//   zpf_candidates(src, n, format, chunk, lanes, cand, cap) -> candidates (cand[0] = 0), or < 0
//   zpf_rules(d, n, lanes, pass, cap, &npass) -> positions where zi_find_header, zi_run or the prefilter disagree
//
// status: 0 ok, -2 no space, -5 preset dictionary, -6 data (the ABI's codes); -100: the lanes disagree (a harness failure).
// Simulated lanes (lanes = 2..64) as in inflate_points_harness.cpp: every lane runs the job over the SAME tables.
#define HARNESS_NAME "points_find_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

struct find_call {
    zi_view<const uint8_t> view;
    zi_tables* S;
    bool header;                               // the test at bit p, or a job
    uint64_t p; zi_find_job job;
    bool ok[MAX_LANES]; zi_find_job res[MAX_LANES];
};
find_call g_call;

void lane_main(int lane)
{
    find_call& c = g_call;
    zi_in_mem in{ c.view };
    if (c.header) c.ok[lane] = zi_find_header(in, c.view, c.p, *c.S, (uint32_t)lane, g_nl);
    else c.res[lane] = zi_find_reach(in, c.view, c.job, *c.S, (uint32_t)lane, g_nl);
}

bool g_disagree = false;

bool test_at(uint64_t p, uint32_t lanes)
{
    g_call.header = true; g_call.p = p;
    memset(g_call.S, 0xA5, sizeof *g_call.S);
    if (!run_lanes(lanes, lane_main)) { g_disagree = true; return false; }
    for (uint32_t l = 1; l < lanes; ++l) if (g_call.ok[l] != g_call.ok[0]) g_disagree = true;
    return g_call.ok[0];
}

zi_find_job run_job(const zi_find_job& j, uint32_t lanes)
{
    g_call.header = false; g_call.job = j;
    memset(g_call.S, 0xA5, sizeof *g_call.S);
    if (!run_lanes(lanes, lane_main)) g_disagree = true;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.res[l].b != g_call.res[0].b || g_call.res[l].c != g_call.res[0].c || g_call.res[l].flags != g_call.res[0].flags) g_disagree = true;
    return g_call.res[0];
}

uint64_t tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }

// k_points_find's result: cand[0] = 0, then the lowest bit of every chunk c >= 1 that passes the prefilter and the test
std::vector<uint64_t> find_candidates(const zi_view<const uint8_t>& view, uint64_t C, uint32_t lanes)
{
    std::vector<uint64_t> cand{ 0 };
    zi_in_mem in{ view };
    const uint64_t chunks = zi_find_chunks(view.n, C);
    for (uint64_t c = 1; c < chunks; ++c) {
        const uint64_t p1 = (c + 1) * C < view.n ? (c + 1) * C * 8 : view.n * 8;
        for (uint64_t p = c * C * 8; p < p1; ++p) {
            if (!zi_find_prefilter_at(in, p)) continue;
            if (test_at(p, lanes)) { cand.push_back(p); break; }
        }
    }
    return cand;
}

}  // namespace

extern "C" int64_t zpf_candidates(const uint8_t* src, uint64_t n, int format, uint64_t C, uint32_t lanes, uint64_t* cand, uint64_t cap)
{
    if (lanes < 1 || lanes > MAX_LANES || C < 16) return -100;
    const int64_t hl = zi_header(format, src, n);
    if (hl < 0 || n - (uint64_t)hl < tlen(format)) return -6;
    std::vector<uint8_t> d(src + hl, src + n);                // exactly D: the checker sees overreads
    std::vector<zi_tables> S(1);
    g_call.view = zi_view<const uint8_t>{ d.data(), d.size() }; g_call.S = &S[0]; g_disagree = false;
    const std::vector<uint64_t> c = find_candidates(g_call.view, C, lanes);
    if (g_disagree) return -100;
    for (uint64_t i = 0; i < c.size() && i < cap; ++i) cand[i] = c[i];
    return (int64_t)c.size();
}

// The whole call. stats[0] candidates, [1] dropped candidates, [2] rounds (launches of the reach jobs), [3] jobs run.
// limit_bytes: 0, or a limit of the test's own -- every job that has a limit gives up that many bytes behind its START, so that
// with a small one the jobs of the true chain give up too and are run again (the call's own limit lies chunk_bytes behind the stop).
extern "C" int zpf_index(const uint8_t* src, uint64_t n, int format, uint64_t C, uint64_t spacing, uint64_t limit_bytes, uint32_t lanes,
                         uint64_t* rows, uint64_t max_entries, uint64_t* entries, uint64_t* out_len, uint64_t* stats)
{
    *entries = 0; *out_len = 0;
    for (int i = 0; i < 4; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES || C < 16 || spacing < 1) return -100;
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return ZI_ITEM_UNSUPPORTED;
    if (hl < 0 || n - (uint64_t)hl < tlen(format)) return ZI_ITEM_DATA;
    std::vector<uint8_t> d(src + hl, src + n);
    const zi_view<const uint8_t> view{ d.data(), d.size() };
    std::vector<zi_tables> S(1);
    g_call.view = view; g_call.S = &S[0]; g_disagree = false;
    const std::vector<uint64_t> cand = find_candidates(view, C, lanes);
    const uint64_t nc = cand.size();
    std::vector<zi_find_job> rc(nc), rr(nc + 1), want(nc + 2);
    std::vector<uint64_t> acc(2 * (2 * nc + 2));
    memset(rc.data(), 0, nc * sizeof(zi_find_job)); memset(rr.data(), 0, (nc + 1) * sizeof(zi_find_job));
    zi_find_walk W{ view_of(cand), nc, zi_view<zi_find_job>{ rc.data(), nc }, zi_view<zi_find_job>{ rr.data(), nc + 1 },
                    zi_view<uint64_t>{ acc.data(), acc.size() }, 0, 0, 0, 0, 0, 0, C };
    uint64_t nwant = nc;
    for (uint64_t k = 0; k < nc; ++k) want[k] = zi_find_first_job(W.cand, nc, k, W.slack, view.n);
    int verdict;
    for (;;) {
        ++stats[2]; stats[3] += nwant;
        if (limit_bytes) for (uint64_t j = 0; j < nwant; ++j) if (want[j].c != ZI_FIND_NONE) want[j].c = want[j].a + 8 * limit_bytes;
        for (uint64_t j = 0; j < nwant; ++j) zi_find_store(W, run_job(want[j], lanes));
        if (g_disagree) return -100;
        verdict = zi_find_link(W, zi_view<zi_find_job>{ want.data(), want.size() }, &nwant);
        if (verdict != ZI_FW_MORE) break;
        if (stats[2] > 3 * nc + 2) return -100;               // (every round confirms a job)
    }
    stats[0] = nc; stats[1] = nc - W.kept;
    if (verdict == ZI_FW_DATA) return ZI_ITEM_DATA;
    uint8_t t[8] = { 0 };
    for (uint64_t i = 0; i < 8 && i < view.n; ++i) t[7 - i] = view[view.n - 1 - i];
    if (!zi_find_trailer_ok(format, view.n, W.end_bit, W.bytes, t)) return ZI_ITEM_DATA;
    *entries = zi_find_rows(W, spacing, nullptr, 0);
    *out_len = W.bytes;
    if (*entries > max_entries) return ZI_ITEM_NOSPACE;
    zi_find_rows(W, spacing, rows, max_entries);
    return ZI_ITEM_OK;
}

// Rule equality over every bit of d[0, n) (raw DEFLATE bytes and whatever follows them): zi_find_header(p) is true iff BFINAL /
// BTYPE at p are 0 / 2 and zi_run from p gets past the header (S.kind == 2 behind a run of one block), and the prefilter rejects
// nothing the test accepts. Returns the positions where either fails (-100: the lanes disagree); pass[0, min(npass, cap)) = the
// positions that pass. With lanes > 1 the test itself runs only where the prefilter or zi_run says yes (elsewhere with one lane).
extern "C" int64_t zpf_rules(const uint8_t* dp, uint64_t n, uint32_t lanes, uint64_t* pass, uint64_t cap, uint64_t* npass)
{
    *npass = 0;
    if (lanes < 1 || lanes > MAX_LANES) return -100;
    std::vector<uint8_t> d(dp, dp + n);
    const zi_view<const uint8_t> view{ d.data(), d.size() };
    std::vector<zi_tables> S(1);
    g_call.view = view; g_call.S = &S[0]; g_disagree = false;
    zi_in_mem in{ view };
    int64_t bad = 0;
    for (uint64_t p = 0; p < n * 8; ++p) {
        const bool pre = zi_find_prefilter_at(in, p);
        bool truth = false;
        if (((in.peek8(p >> 3) >> (p & 7)) & 7u) == 4u) {
            zi_out_count o{ 0 };
            zi_pt_reach pt{ (uint32_t)(p & 7), p + 1, false, 0, ZI_FIND_NONE };
            S[0].kind = 0;
            (void)zi_run(in, view, p >> 3, o, S[0], ZI_RUN_REACH, 0, 0, 1, pt);
            truth = S[0].kind == 2;
        }
        const bool full = test_at(p, (pre || truth) ? lanes : 1);
        if (full != truth || (full && !pre)) ++bad;
        if (full) { if (*npass < cap) pass[*npass] = p; ++*npass; }
    }
    return g_disagree ? -100 : bad;
}
