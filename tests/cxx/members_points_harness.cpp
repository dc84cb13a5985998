// members_points_harness.cpp -- CPU harness of the member point index (zzflate_amd/csrc/zz_inflate_core.h: zi_mf_candidate,
// zi_find_header, zi_mp_measure, zi_mp_link, zi_mp_rows, zi_mp_to_index), the host restatement of zz_members_points_device: the
// header candidates offset by offset (k_members_find_mark), the block candidates chunk by chunk (k_points_find with D = F), the jobs
// of a round last to first (k_members_points_reach), the walk and its repair rounds, the rows. tests/test_members_points_cpu.py
// builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access of the core checked; out of range aborts the
// process) and calls it through ctypes; tests/cxx/members_points_main.cpp is the same code behind a main() for a stand-alone
// sanitizer build.
//
//   zmp_index(src, n, chunk, spacing, own_limit, lanes, rows, max_entries, &entries, &out_len, stats) -> status
//   zmp_candidates(src, n, chunk, lanes, hc, hcap, bc, bcap, counts) -> 0, or < 0
//   zmp_to_index(rows, entries, index, max_entries) -> pairs (0: the rows are no member point index)
//
// zmp_index stats: [0] members, [1] header candidates, [2] block candidates, [3] dropped, [4] rounds, [5] jobs run.
// status: 0 ok, -2 no space, -6 data (the ABI's codes); -100: the lanes disagree (a harness failure).
#define HARNESS_NAME "members_points_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

struct mp_call {
    const uint8_t* src; uint64_t n;
    zi_tables* S;
    int what;                                  // 0: the test at bit p, 1: a job
    uint64_t p; bool ok[MAX_LANES];
    zi_view<const uint64_t> bc; uint64_t nb, C, own_limit;
    zi_mp_job job; zi_mp_job res[MAX_LANES];
};
mp_call g_call;
bool g_disagree = false;

void lane_main(int lane)
{
    mp_call& c = g_call;
    host_lanes w{ (uint32_t)lane };
    const zi_view<const uint8_t> view{ c.src, c.n };
    if (c.what == 0) {
        zi_in_mem in{ view };
        c.ok[lane] = zi_find_header(in, view, c.p, *c.S, (uint32_t)lane, g_nl);
    } else {
        c.res[lane] = zi_mp_measure(w, c.src, c.n, c.bc, c.nb, c.C, c.own_limit, c.job, *c.S, (uint32_t)lane, g_nl);
    }
}

void run(int what, uint32_t lanes)
{
    g_call.what = what;
    memset(g_call.S, 0xA5, sizeof *g_call.S);                 // nothing may rely on what the tables held
    g_call.S->kind = 0;
    if (!run_lanes(lanes, lane_main)) g_disagree = true;
}

bool test_at(uint64_t p, uint32_t lanes)
{
    g_call.p = p;
    run(0, lanes);
    for (uint32_t l = 1; l < lanes; ++l) if (g_call.ok[l] != g_call.ok[0]) g_disagree = true;
    return g_call.ok[0];
}

zi_mp_job measure(const zi_mp_job& j, uint32_t lanes)
{
    g_call.job = j;
    run(1, lanes);
    for (uint32_t l = 1; l < lanes; ++l) {
        const zi_mp_job &a = g_call.res[l], &b = g_call.res[0];
        if (a.b != b.b || a.c != b.c || a.first != b.first || a.flags != b.flags || a.isize != b.isize) g_disagree = true;
    }
    return g_call.res[0];
}

// both candidate lists of F = src[0, n): zi_mf_candidate at every offset; the lowest bit of every chunk c >= 1 that passes the TEST
void candidates(const uint8_t* src, uint64_t n, uint64_t C, uint32_t lanes, std::vector<uint64_t>& hc, std::vector<uint64_t>& bc)
{
    hc.clear(); bc.clear();
    for (uint64_t i = 0; i < n; ++i) if (zi_mf_candidate(src, n, i)) hc.push_back(i);
    const zi_view<const uint8_t> view{ src, n };
    zi_in_mem in{ view };
    const uint64_t chunks = zi_find_chunks(n, C);
    for (uint64_t c = 1; c < chunks; ++c) {
        const uint64_t p1 = (c + 1) * C < n ? (c + 1) * C * 8 : n * 8;
        for (uint64_t p = c * C * 8; p < p1; ++p) {
            if (!zi_find_prefilter_at(in, p)) continue;
            if (test_at(p, lanes)) { bc.push_back(p); break; }
        }
    }
}

}  // namespace

extern "C" int zmp_candidates(const uint8_t* src_in, uint64_t n, uint64_t C, uint32_t lanes, uint64_t* hc_out, uint64_t hcap, uint64_t* bc_out,
                              uint64_t bcap, uint64_t* counts)
{
    if (lanes < 1 || lanes > MAX_LANES || C < 16) return -100;
    std::vector<uint8_t> copy(src_in, src_in + n);            // exactly the file's bytes: the checker sees overreads
    std::vector<zi_tables> S(1);
    g_call.src = copy.data(); g_call.n = n; g_call.S = &S[0]; g_disagree = false;
    std::vector<uint64_t> hc, bc;
    candidates(copy.data(), n, C, lanes, hc, bc);
    if (g_disagree) return -100;
    for (uint64_t i = 0; i < hc.size() && i < hcap; ++i) hc_out[i] = hc[i];
    for (uint64_t i = 0; i < bc.size() && i < bcap; ++i) bc_out[i] = bc[i];
    counts[0] = hc.size(); counts[1] = bc.size();
    return 0;
}

extern "C" int zmp_index(const uint8_t* src_in, uint64_t n, uint64_t C, uint64_t spacing, uint64_t own_limit, uint32_t lanes, uint64_t* rows,
                         uint64_t max_entries, uint64_t* entries, uint64_t* out_len, uint64_t* stats)
{
    *entries = 0; *out_len = 0;
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES || C < 16 || spacing < 1) return -100;
    if (n == 0) return ZI_ITEM_DATA;
    std::vector<uint8_t> copy(src_in, src_in + n);
    std::vector<zi_tables> S(1);
    g_call.src = copy.data(); g_call.n = n; g_call.S = &S[0]; g_disagree = false;
    std::vector<uint64_t> hc, bc;
    candidates(copy.data(), n, C, lanes, hc, bc);
    const uint64_t nh = hc.size(), nb = bc.size();
    g_call.bc = view_of(bc); g_call.nb = nb; g_call.C = C; g_call.own_limit = own_limit;
    std::vector<zi_mp_job> rh(nh + 1), rb(nb + 1), rr(nb + 1), want(nh + nb + 2);
    std::vector<uint64_t> acc(2 * (2 * nh + nb) + 2);
    memset(rh.data(), 0, rh.size() * sizeof(zi_mp_job)); memset(rb.data(), 0, rb.size() * sizeof(zi_mp_job));
    memset(rr.data(), 0, rr.size() * sizeof(zi_mp_job));
    zi_mp_walk W{ view_of(hc), nh, view_of(bc), nb, zi_view<zi_mp_job>{ rh.data(), nh }, zi_view<zi_mp_job>{ rb.data(), nb },
                  zi_view<zi_mp_job>{ rr.data(), nb + 1 }, zi_view<uint64_t>{ acc.data(), 2 * (2 * nh + nb) }, 0, n, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    uint64_t nwant = nh + nb;
    for (uint64_t i = 0; i < nwant; ++i) want[i] = zi_mp_first_job(W, i);
    int verdict;
    for (;;) {
        ++stats[4]; stats[5] += nwant;
        for (uint64_t j = nwant; j-- > 0;) zi_mp_store(W, measure(want[j], lanes));      // (any order: last to first)
        if (g_disagree) return -100;
        verdict = zi_mp_link(W, zi_view<zi_mp_job>{ want.data(), want.size() }, &nwant);
        if (verdict != ZI_FW_MORE) break;
        if (stats[4] > 3 * (nh + nb) + 2) return -100;        // (every round confirms a job)
    }
    stats[0] = W.members; stats[1] = nh; stats[2] = nb; stats[3] = zi_mp_dropped(W);
    if (verdict == ZI_FW_DATA) return ZI_ITEM_DATA;
    *entries = zi_mp_rows(W, spacing, nullptr, 0);
    *out_len = W.bytes;
    if (*entries > max_entries) return ZI_ITEM_NOSPACE;
    zi_mp_rows(W, spacing, rows, max_entries);
    return ZI_ITEM_OK;
}

extern "C" uint64_t zmp_to_index(const uint64_t* rows, uint64_t entries, uint64_t* index, uint64_t max_entries)
{
    return zi_mp_to_index(rows, entries, index, max_entries);
}
