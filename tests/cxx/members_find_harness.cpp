// members_find_harness.cpp -- CPU harness of the members found in parallel (zzflate_amd/csrc/zz_inflate_core.h: zi_mf_candidate,
// zi_mf_measure, zi_mf_link, zi_mf_again, zi_mf_dealt, zi_mf_is_mstar), the host restatement of zz_members_find_device and
// zz_decode_members_found_device: the candidates offset by offset (k_members_find_mark), the measures of a round with their limit
// (k_members_reach), the walk, round 2, the slots (k_members_find_slots), zi_item per dealt member and zi_members where the
// procedure says so. tests/test_members_find_cpu.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer
// access of the core checked; out of range aborts the process) and calls it through ctypes; tests/cxx/members_find_main.cpp is the
// same code behind a main() for a stand-alone sanitizer build.
//
//   zmf_find(src, n, limit_bytes, lanes, rows, max_entries, &entries, stats) -> status
//   zmf_decode(src, n, out, cap, limit_bytes, lanes, &out_len, stats) -> status
//   zmf_candidates(src, n, cand, cap) -> candidates
//
// stats[0] members, [1] candidates, [2] dropped, [3] rounds, [4] jobs run. status: 0 ok, -2 no space, -6 data (the ABI's codes);
// -100: the lanes disagree (a harness failure). Simulated lanes (lanes = 2..64) as in inflate_members_harness.cpp.
#define HARNESS_NAME "members_find_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

struct find_call {
    const uint8_t* src; uint64_t n;
    zi_tables* S;
    int what;                                  // 0: a measure, 1: zi_item on a cut-out member, 2: zi_members
    zi_find_job job; zi_find_job res[MAX_LANES];
    const uint8_t* isrc; uint64_t ilen; uint8_t* out; uint64_t cap;
    zi_item_result ires[MAX_LANES]; zi_members_result mres[MAX_LANES];
};
find_call g_call;
bool g_disagree = false;

void lane_main(int lane)
{
    find_call& c = g_call;
    host_lanes w{ (uint32_t)lane };
    if (c.what == 0) c.res[lane] = zi_mf_measure(w, c.src, c.n, c.job, *c.S, (uint32_t)lane, g_nl);
    else if (c.what == 1) c.ires[lane] = zi_item(w, c.isrc, c.ilen, c.out, c.cap, 1, *c.S, (uint32_t)lane, g_nl);
    else c.mres[lane] = zi_members(w, c.isrc, c.ilen, c.out, c.cap, *c.S, (uint32_t)lane, g_nl);
}

void run(int what, uint32_t lanes)
{
    g_call.what = what;
    memset(g_call.S, 0xA5, sizeof *g_call.S);                 // nothing may rely on what the tables held
    if (!run_lanes(lanes, lane_main)) g_disagree = true;
}

zi_find_job measure(const zi_find_job& j, uint32_t lanes)
{
    g_call.job = j;
    run(0, lanes);
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.res[l].b != g_call.res[0].b || g_call.res[l].c != g_call.res[0].c || g_call.res[l].flags != g_call.res[0].flags) g_disagree = true;
    return g_call.res[0];
}

zi_item_result item(const uint8_t* p, uint64_t len, uint8_t* out, uint64_t cap, uint32_t lanes)
{
    std::vector<uint8_t> cut(p, p + len);                     // exactly the member's bytes
    cut.push_back(0);
    g_call.isrc = cut.data(); g_call.ilen = len; g_call.out = out; g_call.cap = cap;
    run(1, lanes);
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.ires[l].status != g_call.ires[0].status || g_call.ires[l].out != g_call.ires[0].out) g_disagree = true;
    return g_call.ires[0];
}

zi_members_result members(const uint8_t* p, uint64_t len, uint8_t* out, uint64_t cap, uint32_t lanes)
{
    g_call.isrc = p; g_call.ilen = len; g_call.out = out; g_call.cap = cap;
    run(2, lanes);
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.mres[l].status != g_call.mres[0].status || g_call.mres[l].out != g_call.mres[0].out || g_call.mres[l].members != g_call.mres[0].members)
            g_disagree = true;
    return g_call.mres[0];
}

// the front of both calls: candidates, round 1, the walk, round 2, the walk again. Returns ZI_MF_CLEAN or ZI_MF_BROKEN.
int front(const uint8_t* src, uint64_t n, uint64_t limit_bytes, uint32_t lanes, std::vector<zi_find_job>& rec, std::vector<uint8_t>& keep,
          uint64_t* stats)
{
    g_call.src = src; g_call.n = n;
    std::vector<uint64_t> cand;
    for (uint64_t i = 0; i < n; ++i) if (zi_mf_candidate(src, n, i)) cand.push_back(i);
    const uint64_t nc = cand.size();
    rec.assign(nc, zi_find_job{ 0, 0, 0, 0, 0 }); keep.assign(nc, 0);
    stats[1] = nc;
    for (uint64_t k = nc; k-- > 0;) rec[k] = measure(zi_find_job{ cand[k], 0, zi_mf_limit(k, limit_bytes), 0, 0 }, lanes);   // (any order)
    stats[3] = 1; stats[4] = nc;
    zi_mf_walk W{ 0, 0, 0, 0 };
    const zi_view<const zi_find_job> recs{ rec.data(), nc };
    int v = zi_mf_link(W, recs, nc, n, zi_view<uint8_t>{ keep.data(), nc });
    if (v == ZI_MF_MORE) {
        std::vector<uint32_t> which(zi_mf_again(W, recs, nc, nullptr) + 1);
        const uint64_t nw = zi_mf_again(W, recs, nc, which.data());
        for (uint64_t i = 0; i < nw; ++i) rec[which[i]] = measure(zi_find_job{ cand[which[i]], 0, ZI_FIND_NONE, 0, 0 }, lanes);
        stats[3] = 2; stats[4] += nw;
        v = zi_mf_link(W, recs, nc, n, zi_view<uint8_t>{ keep.data(), nc });
        if (v == ZI_MF_MORE) g_disagree = true;               // (a job without a limit does not give up)
    }
    stats[0] = W.members; stats[2] = W.dropped;
    return v;
}

}  // namespace

extern "C" int64_t zmf_candidates(const uint8_t* src_in, uint64_t n, uint64_t* cand, uint64_t cap)
{
    std::vector<uint8_t> copy(src_in, src_in + n);            // exactly the file's bytes: the checker sees overreads
    copy.push_back(0);
    const uint8_t* src = copy.data();
    uint64_t nc = 0;
    for (uint64_t i = 0; i < n; ++i) if (zi_mf_candidate(src, n, i)) { if (nc < cap) cand[nc] = i; ++nc; }
    return (int64_t)nc;
}

extern "C" int zmf_find(const uint8_t* src_in, uint64_t n, uint64_t limit_bytes, uint32_t lanes, uint64_t* rows, uint64_t max_entries,
                        uint64_t* entries, uint64_t* stats)
{
    *entries = 0;
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES || limit_bytes == 0) return -100;
    if (n == 0) return ZI_ITEM_DATA;
    std::vector<uint8_t> copy(src_in, src_in + n);
    std::vector<zi_tables> S(1);
    g_call.S = &S[0]; g_disagree = false;
    std::vector<zi_find_job> rec; std::vector<uint8_t> keep;
    const int v = front(copy.data(), n, limit_bytes, lanes, rec, keep, stats);
    if (g_disagree) return -100;
    if (v != ZI_MF_CLEAN) return ZI_ITEM_DATA;
    *entries = stats[0] + 1;
    if (*entries > max_entries) return ZI_ITEM_NOSPACE;
    uint64_t j = 0, off = 0;
    for (uint64_t k = 0; k < rec.size(); ++k) {
        if (!keep[k]) continue;
        rows[2 * j] = rec[k].a; rows[2 * j + 1] = off;
        off += rec[k].c; ++j;
    }
    rows[2 * j] = n; rows[2 * j + 1] = off;
    return ZI_ITEM_OK;
}

extern "C" int zmf_decode(const uint8_t* src_in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t limit_bytes, uint32_t lanes,
                          uint64_t* out_len, uint64_t* stats)
{
    *out_len = ~0ull;
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES || limit_bytes == 0) return -100;
    if (n == 0) return ZI_ITEM_DATA;
    std::vector<uint8_t> copy(src_in, src_in + n);
    const uint8_t* src = copy.data();
    std::vector<zi_tables> S(1);
    g_call.S = &S[0]; g_disagree = false;
    const auto serial = [&](uint64_t at, uint64_t off) -> int {
        const zi_members_result R = members(src + at, n - at, out + off, cap - off, lanes);
        if (g_disagree) return -100;
        if (R.status == ZI_ITEM_OK) *out_len = off + R.out;
        return R.status;
    };
    std::vector<zi_find_job> rec; std::vector<uint8_t> keep;
    const int v = front(src, n, limit_bytes, lanes, rec, keep, stats);
    if (g_disagree) return -100;
    if (v != ZI_MF_CLEAN) return serial(0, 0);
    // the slots, and zi_item over the members in front of m*: the first that does not answer OK, or m*, is where zi_members begins
    uint64_t off = 0;
    for (uint64_t k = 0; k < rec.size(); ++k) {
        if (!keep[k]) continue;
        const uint64_t c = rec[k].a, used = rec[k].b, o = rec[k].c;
        if (zi_mf_is_mstar(o, off, cap)) return serial(c, off);
        if (!zi_mf_dealt(o, off, cap)) return -100;            // (members behind m* are not reached)
        const zi_item_result r = item(src + c, used, out + off, o, lanes);
        if (g_disagree) return -100;
        if (r.status != ZI_ITEM_OK) return serial(c, off);
        off += o;
    }
    *out_len = off;
    return ZI_ITEM_OK;
}
