// inflate_members_harness.cpp -- CPU harness of the member-file rules (zzflate_amd/csrc/zz_inflate_core.h): zi_members, the
// routine k_inflate_members runs and the definition of zz_decode_members_device's result; zi_bc_len; and a host restatement
// of the blocked path -- candidates, chain check, hop, slots, zi_item per dealt member, verdict, re-judging -- with the very functions the
// kernels of zz_inflate_members.h call. tests/test_inflate_members_cpu.py builds it with g++ -fsanitize=undefined
// -DZZ_INFLATE_CHECKED (every buffer access of the core checked; out of range aborts the process) and calls it through ctypes.
//
//   zmt_members(src, n, out, cap, lanes, &out_len, &members) -> status     lanes = 1, or 2..64 simulated lanes
//   zmt_bc_len(h, n) -> announced member length or 0
//   zmt_blocked(src, n, out, cap, &out_len, &members, &candidates, &path) -> status    path as the C ABI reports it
//
// Simulated lanes are those of inflate_items_harness.cpp: every lane is a coroutine running the routine with its own lane
// number over the same tables and destination, and the lanes meet, round robin, wherever a wavefront's lanes depend on what
// other lanes wrote.
#define HARNESS_NAME "inflate_members_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

struct call {
    const uint8_t* src; uint64_t n; uint8_t* out; uint64_t cap;
    zi_tables* S;
    zi_members_result res[MAX_LANES];
};
call g_call;

void lane_main(int lane)
{
    host_lanes w{ (uint32_t)lane };
    g_call.res[lane] = zi_members(w, g_call.src, g_call.n, g_call.out, g_call.cap, *g_call.S, (uint32_t)lane, g_nl);
}

}  // namespace

// status: 0 ok, -2 no space, -6 data (the ABI's codes); -100: the lanes disagree (a harness failure)
extern "C" int zmt_members(const uint8_t* src, uint64_t n, uint8_t* out, uint64_t cap, uint32_t lanes, uint64_t* out_len, uint64_t* members)
{
    *out_len = 0; *members = 0;
    if (lanes < 1 || lanes > MAX_LANES) return -100;
    std::vector<uint8_t> copy(src, src + n);                  // exactly the file's bytes
    zi_tables* S = new zi_tables();
    memset(S, 0xA5, sizeof *S);                               // nothing may rely on what the tables held
    g_call = call{ copy.data(), n, out, cap, S, {} };
    if (!run_lanes(lanes, lane_main)) { delete S; return -100; }
    delete S;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.res[l].status != g_call.res[0].status || g_call.res[l].out != g_call.res[0].out ||
            g_call.res[l].members != g_call.res[0].members) return -100;
    *out_len = g_call.res[0].out; *members = g_call.res[0].members;
    return g_call.res[0].status;
}

extern "C" uint32_t zmt_bc_len(const uint8_t* h, uint64_t n)
{
    std::vector<uint8_t> copy(h, h + n);
    return zi_bc_len(copy.data(), n);
}

// zz_decode_members_device's procedure on the host, one lane: mark, check, hop, slots, zi_item per dealt member, verdict, and
// the serial path where the procedure says so
extern "C" int zmt_blocked(const uint8_t* src_in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* members,
                           uint64_t* candidates, int* path)
{
    *out_len = 0; *members = 0; *candidates = 0; *path = 0;
    if (n == 0) return ZI_ITEM_DATA;
    std::vector<uint8_t> copy(src_in, src_in + n);
    const uint8_t* src = copy.data();
    const auto serial = [&]() -> int {
        *path = 3;
        return zmt_members(src, n, out, cap, 1, out_len, members);
    };
    std::vector<uint64_t> offs; std::vector<uint32_t> lens;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t len = zi_members_candidate(src, n, i);
        if (len) { offs.push_back(i); lens.push_back(len); }
    }
    const uint64_t ncand = offs.size();
    *candidates = ncand;
    if (ncand == 0) return serial();
    bool chain_bad = false;
    for (uint64_t j = 0; j < ncand; ++j)
        if (zi_members_link_broken(j, ncand, offs[j], lens[j], j + 1 < ncand ? offs[j + 1] : 0, n)) chain_bad = true;
    uint64_t m = ncand;
    if (chain_bad) m = zi_members_hop(src, n, offs.data(), lens.data(), ncand);
    if (m == 0) return serial();
    uint64_t off = 0, mstar = ~0ull, mstar_src = 0, mstar_dst = 0, n_data = 0, n_nospace = 0, dealt = 0;
    zi_tables* S = new zi_tables();
    host_lanes w{ 0 };
    g_sim = false; g_nl = 1;
    for (uint64_t j = 0; j < m && mstar == ~0ull; ++j) {
        const uint32_t isize = zi_members_isize(zi_view<const uint8_t>{ src, n }, offs[j], lens[j]);
        if (zi_members_is_mstar(isize, off, cap)) { mstar = j; mstar_src = offs[j]; mstar_dst = off; }
        std::vector<uint8_t> item(src + offs[j], src + offs[j] + lens[j]);      // exactly the member's bytes
        const zi_item_result r = zi_item(w, item.data(), lens[j], out + off, zi_members_slot_cap(isize, off, cap), 1, *S, 0, 1);
        if (r.status == ZI_ITEM_NOSPACE) ++n_nospace;
        else if (r.status != ZI_ITEM_OK) ++n_data;
        off += isize; ++dealt;
    }
    delete S;
    const int v = zi_members_verdict(mstar != ~0ull, n_data, n_nospace);
    if (v == ZI_MEMBERS_SERIAL) return serial();
    *path = chain_bad ? 2 : 1;
    if (v == ZI_MEMBERS_REJUDGE) {
        // "no space" from the cut-out m* is a claim: the serial rule from m* on, over what is left of source and room, decides
        uint64_t tail_out = 0, tail_members = 0;
        const int rc = zmt_members(src + mstar_src, n - mstar_src, out + mstar_dst, cap - mstar_dst, 1, &tail_out, &tail_members);
        *members = mstar + tail_members;
        if (rc == ZI_ITEM_OK) *out_len = mstar_dst + tail_out;
        else if (rc != ZI_ITEM_NOSPACE) *path = 3;
        return rc;
    }
    *members = dealt; *out_len = off;
    return v;
}
