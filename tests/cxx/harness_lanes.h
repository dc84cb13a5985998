// harness_lanes.h -- what the CPU harnesses of the inflate core (zzflate_amd/csrc/zz_inflate_core.h) share: the core's lane
// group on the host (host_in, host_fence, host_lanes, view_of) and the simulated lanes. The including file sets HARNESS_NAME
// (the abort messages name the harness) and includes this INSTEAD of the core: ZI_LANES_SYNC is defined here, in front of it.
//
// Simulated lanes: every lane is a coroutine (ucontext) running the same body with its own lane number over the SAME tables and
// the same destination, as the lanes of a wavefront do. A wavefront's lanes run in lockstep; here a lane runs alone until it
// reaches a point where it depends on what other lanes wrote -- ZI_LANES_SYNC() in the table builder, the output policy's fence
// in front of a match copy, the sync in front of the checksum, a sum over the lanes -- and there the next lane runs, round
// robin: a barrier. Between two barriers the lanes only repeat identical writes or write disjoint places, as on the device.
// With one lane nothing is simulated (g_sim == false): the barrier returns at once and a sum is its own value.
#pragma once
#ifndef HARNESS_NAME
#error "define HARNESS_NAME before including harness_lanes.h"
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ucontext.h>
#include <vector>

inline void lanes_sync();
#define ZI_LANES_SYNC() lanes_sync()
#include "../../zzflate_amd/csrc/zz_inflate_core.h"

constexpr uint32_t MAX_LANES = 64;
constexpr size_t STACK_BYTES = 256 * 1024;

struct lane_state {
    ucontext_t ctx;
    bool done;
};
inline lane_state g_lane[MAX_LANES];
inline ucontext_t g_main;
inline uint32_t g_nl = 1, g_cur = 0;
inline bool g_sim = false;
inline uint64_t g_slot[MAX_LANES];
inline std::vector<uint8_t> g_stacks;
inline void (*g_body)(int) = nullptr;

// the barrier: hand over to the next lane; it comes back here when every other lane has reached its own call
inline void lanes_sync()
{
    if (!g_sim) return;
    const uint32_t me = g_cur, nx = (me + 1) % g_nl;
    if (g_lane[nx].done) { fprintf(stderr, HARNESS_NAME ": the lanes left their lockstep\n"); abort(); }
    g_cur = nx;
    swapcontext(&g_lane[me].ctx, &g_lane[nx].ctx);
}

inline void lane_entry(int lane)
{
    g_body(lane);
    g_lane[lane].done = true;
    // (returns to g_main through uc_link)
}

__attribute__((noinline)) inline void make_lane(uint32_t l)
{
    g_lane[l].done = false;
    getcontext(&g_lane[l].ctx);
    g_lane[l].ctx.uc_stack.ss_sp = g_stacks.data() + (size_t)l * STACK_BYTES;
    g_lane[l].ctx.uc_stack.ss_size = STACK_BYTES;
    g_lane[l].ctx.uc_link = &g_main;
    makecontext(&g_lane[l].ctx, (void (*)())lane_entry, 1, (int)l);
}

// runs body(lane) for lanes 0 .. lanes - 1 (1 .. MAX_LANES); false: a lane did not finish (a harness failure)
inline bool run_lanes(uint32_t lanes, void (*body)(int))
{
    g_nl = lanes;
    if (lanes == 1) { g_sim = false; body(0); return true; }
    g_sim = true;
    g_body = body;
    if (g_stacks.size() < MAX_LANES * STACK_BYTES) g_stacks.resize(MAX_LANES * STACK_BYTES);
    for (uint32_t l = 0; l < lanes; ++l) make_lane(l);
    // the lanes are in lockstep, so when one returns all the others stand at their last barrier: finish them in order
    for (uint32_t l = 0; l < lanes; ++l) {
        if (g_lane[l].done) continue;
        g_cur = l;
        swapcontext(&g_main, &g_lane[l].ctx);
    }
    g_sim = false;
    for (uint32_t l = 0; l < lanes; ++l) if (!g_lane[l].done) return false;
    return true;
}

// the core's input, fence and lane group on the host
struct host_in {
    zz::zi_view<const uint8_t> v;
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
    in_t input(const uint8_t* p, uint64_t n) const { return in_t{ zz::zi_view<const uint8_t>{ p, n } }; }
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

template <class T> zz::zi_view<const T> view_of(const std::vector<T>& v) { return zz::zi_view<const T>{ v.data(), v.size() }; }
