// inflate_items_harness.cpp -- CPU harness of zi_item (zzflate_amd/csrc/zz_inflate_core.h): the routine k_inflate_items runs
// per stream of a batch -- container header, blocks, trailer and checksum by one group of lanes. tests/test_inflate_items_cpu.py
// builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access of the core checked; out of range aborts
// the process) and calls it through ctypes.
//
//   zit_item(src, n, format, out, cap, lanes, &out_len) -> status     lanes = 1, or 2..64 simulated lanes
//
// Simulated lanes: every lane is a coroutine (ucontext) running zi_item with its own lane number over the SAME tables and the
// same destination, as the lanes of a wavefront do. A wavefront's lanes run in lockstep; here a lane runs alone until it reaches
// a point where it depends on what other lanes wrote -- ZI_LANES_SYNC() in the table builder, the output policy's fence in front
// of a match copy, the sync in front of the checksum, a sum over the lanes -- and there the next lane runs, round robin: a
// barrier. Between two barriers the lanes only repeat identical writes or write disjoint places, as on the device.
#define HARNESS_NAME "inflate_items_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

struct call {
    const uint8_t* src; uint64_t n; int format; uint8_t* out; uint64_t cap;
    zi_tables* S;
    zi_item_result res[MAX_LANES];
};
call g_call;

void lane_main(int lane)
{
    host_lanes w{ (uint32_t)lane };
    g_call.res[lane] = zi_item(w, g_call.src, g_call.n, g_call.out, g_call.cap, g_call.format, *g_call.S, (uint32_t)lane, g_nl);
}

}  // namespace

// status: 0 ok, -2 no space, -5 preset dictionary, -6 data (the ABI's codes); -100: the lanes disagree (a harness failure)
extern "C" int zit_item(const uint8_t* src, uint64_t n, int format, uint8_t* out, uint64_t cap, uint32_t lanes, uint64_t* out_len)
{
    *out_len = 0;
    if (lanes < 1 || lanes > MAX_LANES) return -100;
    std::vector<uint8_t> copy(src, src + n);                  // exactly the item's bytes: the checker sees overreads
    zi_tables* S = new zi_tables();
    memset(S, 0xA5, sizeof *S);                               // nothing may rely on what the tables held
    g_call = call{ copy.data(), n, format, out, cap, S, {} };
    if (!run_lanes(lanes, lane_main)) { delete S; return -100; }
    delete S;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.res[l].status != g_call.res[0].status || g_call.res[l].out != g_call.res[0].out) return -100;
    *out_len = g_call.res[0].out;
    return g_call.res[0].status;
}
