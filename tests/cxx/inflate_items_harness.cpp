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
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ucontext.h>
#include <vector>

namespace { void lanes_sync(); }
#define ZI_LANES_SYNC() lanes_sync()
#include "../../zzflate_amd/csrc/zz_inflate_core.h"

using namespace zz;

namespace {

constexpr uint32_t MAX_LANES = 64;
constexpr size_t STACK_BYTES = 256 * 1024;

struct lane_state {
    ucontext_t ctx;
    bool done;
};
lane_state g_lane[MAX_LANES];
ucontext_t g_main;
uint32_t g_nl = 1, g_cur = 0;
bool g_sim = false;
uint64_t g_slot[MAX_LANES];
std::vector<uint8_t> g_stacks;

// the barrier: hand over to the next lane; it comes back here when every other lane has reached its own call
void lanes_sync()
{
    if (!g_sim) return;
    const uint32_t me = g_cur, nx = (me + 1) % g_nl;
    if (g_lane[nx].done) { fprintf(stderr, "inflate_items_harness: the lanes left their lockstep\n"); abort(); }
    g_cur = nx;
    swapcontext(&g_lane[me].ctx, &g_lane[nx].ctx);
}

struct host_in {
    zi_view<const uint8_t> v;
    uint64_t peek8(uint64_t pos) const
    {
        uint64_t r = 0;
        for (uint32_t i = 0; i < 8; ++i) if (pos + i < v.n) r |= (uint64_t)v[pos + i] << (8 * i);
        return r;
    }
};
struct host_fence { void operator()() const { lanes_sync(); } };
struct host_lanes {
    typedef host_in in_t;
    typedef host_fence fence_t;
    uint32_t lane;
    in_t input(const uint8_t* p, uint64_t n) const { return in_t{ zi_view<const uint8_t>{ p, n } }; }
    void sync() const { lanes_sync(); }
    uint64_t sum(uint64_t v) const
    {
        if (!g_sim) return v;
        g_slot[lane] = v;
        lanes_sync();
        uint64_t s = 0;
        for (uint32_t i = 0; i < g_nl; ++i) s += g_slot[i];
        lanes_sync();                                         // every lane has read the slots
        return s;
    }
    uint32_t fold_xor(uint32_t v) const
    {
        if (!g_sim) return v;
        g_slot[lane] = v;
        lanes_sync();
        uint32_t s = 0;
        for (uint32_t i = 0; i < g_nl; ++i) s ^= (uint32_t)g_slot[i];
        lanes_sync();
        return s;
    }
};

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
    g_lane[lane].done = true;
    // (returns to g_main through uc_link)
}

__attribute__((noinline)) void make_lane(uint32_t l)
{
    g_lane[l].done = false;
    getcontext(&g_lane[l].ctx);
    g_lane[l].ctx.uc_stack.ss_sp = g_stacks.data() + (size_t)l * STACK_BYTES;
    g_lane[l].ctx.uc_stack.ss_size = STACK_BYTES;
    g_lane[l].ctx.uc_link = &g_main;
    makecontext(&g_lane[l].ctx, (void (*)())lane_main, 1, (int)l);
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
    g_nl = lanes;
    if (lanes == 1) {
        g_sim = false;
        lane_main(0);
    } else {
        g_sim = true;
        if (g_stacks.size() < MAX_LANES * STACK_BYTES) g_stacks.resize(MAX_LANES * STACK_BYTES);
        for (uint32_t l = 0; l < lanes; ++l) make_lane(l);
        // the lanes are in lockstep, so when one returns all the others stand at their last barrier: finish them in order
        for (uint32_t l = 0; l < lanes; ++l) {
            if (g_lane[l].done) continue;
            g_cur = l;
            swapcontext(&g_main, &g_lane[l].ctx);
        }
        g_sim = false;
        for (uint32_t l = 0; l < lanes; ++l) if (!g_lane[l].done) { delete S; return -100; }
    }
    delete S;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.res[l].status != g_call.res[0].status || g_call.res[l].out != g_call.res[0].out) return -100;
    *out_len = g_call.res[0].out;
    return g_call.res[0].status;
}
