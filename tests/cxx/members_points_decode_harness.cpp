// members_points_decode_harness.cpp -- CPU harness of the decode through a member point index (zzflate_amd/csrc/zz_inflate_core.h:
// zi_mpd_plan, zi_mpd_mstar, zi_mpd_batch, zi_mpd_segment, zi_mpd_fold_run, zi_mpd_fold_step, zi_mpd_verdict), the host restatement
// of zz_decode_members_points_device: the check of the rows, the descriptors and the batches, phase 1 per descriptor
// (k_members_segments, with zi_out_segment<.., zi_bits_plain>), the rounds as inflate_points_harness.cpp restates them
// (k_inflate_resolve's rule, a round reading what the round before left), the sums (k_members_sums), the verdict per member with
// its runs and its tree (k_members_verdict) and the serial tail through zi_members (k_inflate_members).
// tests/members_points_decode_cases.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED (every buffer access of the
// core checked; out of range aborts the process) and calls it through ctypes; tests/cxx/members_points_decode_main.cpp is the same
// code behind a main() for a stand-alone sanitizer build.
//
//   zmpd_decode(src, n, rows, entries, out, cap, batch_bytes, lanes, &out_len, stats) -> status
//
// status: 0 ok, -2 no space, -6 data (the ABI's codes); -100: the lanes disagree, a host loop passed its iteration cap, or the
// bitmap does not hold what the lanes counted (a harness failure). `out` has `cap` bytes and the harness writes nowhere else.
// stats: [0] members the rows name, [1] members proven in front of the serial tail, [2] segments dealt, [3] batches, [4] pending
// bytes, [5] rounds (the most of any batch), [6] 1: the serial path ran, [7] the most turns any host loop took.
// The host loops and their caps: the plan (one row per turn: entries), m* (one member per turn), the batches (at least one
// descriptor per turn: the dealt descriptors), a batch's inner loop (the dealt descriptors).
#define HARNESS_NAME "members_points_decode_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

struct mpd_call {
    const uint8_t* src; uint64_t n;
    zi_mpd_seg d;
    uint8_t* dst; uint64_t base, nbytes;
    uint32_t* st; uint32_t* pend; uint64_t words;
    zi_tables* S;
    int what;                                  // 0: a descriptor's phase 1, 1: its sum, 2: the serial tail
    zi_result res[MAX_LANES]; uint32_t npend[MAX_LANES];
    uint32_t sum[MAX_LANES];
    const uint8_t* tsrc; uint64_t tn; uint8_t* tdst; uint64_t tcap;
    zi_members_result tail[MAX_LANES];
};
mpd_call g_call;

void lane_main(int lane)
{
    mpd_call& c = g_call;
    host_lanes w{ (uint32_t)lane };
    if (c.what == 0) {
        zi_in_mem in{ zi_view<const uint8_t>{ c.src, c.n } };
        c.res[lane] = zi_mpd_segment<host_fence, zi_bits_plain>(in, c.src, c.n, c.d, c.dst, c.base, c.pend, c.words, c.st, c.nbytes, *c.S,
                                                                (uint32_t)lane, g_nl, &c.npend[lane]);
    } else if (c.what == 1) {
        const uint64_t len = c.d.o1 - c.d.o0;
        c.sum[lane] = zi_crc_lanes(w, zi_view<const uint8_t>{ c.dst + c.d.o0, len }, len, (uint32_t)lane, g_nl);
    } else {
        c.tail[lane] = zi_members(w, c.tsrc, c.tn, c.tdst, c.tcap, *c.S, (uint32_t)lane, g_nl);
    }
}

bool run(int what, uint32_t lanes)
{
    g_call.what = what;
    memset(g_call.S, 0xA5, sizeof *g_call.S);                 // nothing may rely on what the tables held
    g_call.S->kind = 0;
    return run_lanes(lanes, lane_main);
}

// zi_members over src[at, n) onto out[off, cap): the serial path's answer
int serial(const uint8_t* src, uint64_t n, uint64_t at, uint8_t* out, uint64_t off, uint64_t cap, uint32_t lanes, uint64_t* out_len)
{
    std::vector<uint8_t> copy(src + at, src + n);             // exactly what is left of the file: the checker sees overreads
    copy.push_back(0);
    g_call.tsrc = copy.data(); g_call.tn = n - at; g_call.tdst = out + off; g_call.tcap = cap - off;
    if (!run(2, lanes)) return -100;
    for (uint32_t l = 1; l < lanes; ++l)
        if (g_call.tail[l].status != g_call.tail[0].status || g_call.tail[l].out != g_call.tail[0].out) return -100;
    if (g_call.tail[0].status == ZI_ITEM_OK) *out_len = off + g_call.tail[0].out;
    return g_call.tail[0].status;
}

}  // namespace

extern "C" int zmpd_decode(const uint8_t* src_in, uint64_t n, const uint64_t* rows, uint64_t entries, uint8_t* out, uint64_t cap,
                           uint64_t batch_bytes, uint32_t lanes, uint64_t* out_len, uint64_t* stats)
{
    *out_len = ~0ull;
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (lanes < 1 || lanes > MAX_LANES || batch_bytes > (64ull << 20)) return -100;
    if (n == 0) return ZI_ITEM_DATA;
    const uint64_t limit = batch_bytes ? batch_bytes : (64ull << 20);
    std::vector<uint8_t> copy(src_in, src_in + n);            // exactly the file's bytes
    const uint8_t* src = copy.data();
    std::vector<zi_tables> S(1);
    g_call.src = src; g_call.n = n; g_call.S = &S[0]; g_call.dst = out;
    const auto tail = [&](uint64_t proven, uint64_t at, uint64_t off) {
        stats[1] = proven; stats[6] = 1;
        return serial(src, n, at, out, off, cap, lanes, out_len);
    };
    uint64_t nmem = 0, nseg = 0;
    if (!zi_mpd_plan(rows, entries, n, nullptr, 0, nullptr, 0, &nmem, &nseg)) return tail(0, 0, 0);
    if (nmem > entries || nseg > entries) return -100;        // (the plan's loop: one row per turn)
    stats[7] = entries;
    std::vector<zi_mpd_member> mem(nmem);
    std::vector<zi_mpd_seg> seg(nseg + 1);
    zi_mpd_plan(rows, entries, n, mem.data(), nmem, seg.data(), nseg, &nmem, &nseg);
    stats[0] = nmem;
    const uint64_t mstar = zi_mpd_mstar(mem.data(), nmem, cap, limit);
    if (mstar > nmem) return -100;
    const uint64_t dealt = mstar, dsegs = mstar < nmem ? mem[mstar].seg0 : nseg;
    stats[2] = dsegs;
    if (dealt == 0) return tail(0, 0, 0);
    std::vector<uint8_t> segok(dsegs, 0);
    std::vector<uint32_t> sums(dsegs, 0xDEADBEEFu);
    uint64_t turns = 0;
    bool refused = false;
    for (uint64_t k0 = 0, k1; k0 < dsegs && !refused; k0 = k1) {
        k1 = zi_mpd_batch(seg.data(), dsegs, k0, limit, 1u << 20);
        if (k1 <= k0 || k1 > dsegs || ++turns > dsegs) return -100;           // a batch takes at least one descriptor
        ++stats[3];
        const uint64_t base = seg[k0].o0, nbytes = seg[k1 - 1].o1 - base;
        if (nbytes > limit || base + nbytes > cap) return -100;               // a batch holds at most `limit` bytes, inside the destination
        const uint64_t tiles = (nbytes + ZI_POINTS_TILE - 1) / ZI_POINTS_TILE, words = tiles * (ZI_POINTS_TILE / 32);
        std::vector<uint32_t> st(nbytes + 1, 0), pend(words + 1, 0), pcnt(tiles + 1, 0);
        g_call.base = base; g_call.nbytes = nbytes; g_call.st = st.data(); g_call.pend = pend.data(); g_call.words = words;
        for (uint64_t k = k0; k < k1; ++k) {                  // phase 1
            g_call.d = seg[k];
            if (!run(0, lanes)) return -100;
            for (uint32_t l = 1; l < lanes; ++l)
                if (g_call.res[l].err != g_call.res[0].err || g_call.res[l].out != g_call.res[0].out || g_call.res[l].final != g_call.res[0].final) return -100;
            if (g_call.res[0].err) { refused = true; continue; }
            segok[k] = 1;
        }
        // the tile counts and the rounds, also in a batch that holds refused segments: pointers never leave their member
        uint64_t batch_pend = 0;
        for (uint64_t t = 0; t < tiles; ++t) {
            uint32_t c = 0;
            for (uint32_t w = 0; w < ZI_POINTS_TILE / 32; ++w) c += zi_popc32(pend[t * (ZI_POINTS_TILE / 32) + w]);
            pcnt[t] = c; batch_pend += c;
        }
        if (batch_pend) {
            stats[4] += batch_pend;
            auto pending = [&](uint64_t x) { return pcnt[x / ZI_POINTS_TILE] && ((pend[x >> 5] >> (x & 31)) & 1u); };
            std::vector<uint64_t> open, still;
            for (uint64_t x = 0; x < nbytes; ++x) if (pending(x)) open.push_back(x);
            std::vector<uint32_t> adopted;
            std::vector<uint8_t> done_round(nbytes, 0);
            for (uint32_t round = 1;; ++round) {
                still.clear(); adopted.clear();
                for (const uint64_t x : open) {
                    const int64_t y = (int64_t)(st[x] & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
                    if ((int64_t)base + y < 0 || y >= (int64_t)x) return -100;            // in front of the file's bytes, or not in front of x
                    if (y < 0 || !pending((uint64_t)y) || (done_round[(uint64_t)y] && done_round[(uint64_t)y] < round)) {
                        out[base + x] = out[(int64_t)base + y]; done_round[x] = (uint8_t)round;
                    } else { still.push_back(x); adopted.push_back(st[(uint64_t)y]); }
                }
                for (uint64_t i = 0; i < still.size(); ++i) st[still[i]] = adopted[i];
                open.swap(still);
                if (open.empty()) { if (round > stats[5]) stats[5] = round; break; }
                if (round > ZI_ROUND_EXTERNAL - 1) return -100;
            }
        }
        for (uint64_t k = k0; k < k1; ++k) {                  // the sums
            g_call.d = seg[k];
            if (!run(1, lanes)) return -100;
            for (uint32_t l = 1; l < lanes; ++l) if (g_call.sum[l] != g_call.sum[0]) return -100;
            sums[k] = g_call.sum[0];
        }
    }
    if (turns > stats[7]) stats[7] = turns;
    // the verdict: per dealt member 64 runs and six steps of the tree, whatever `lanes` is (the kernel's lanes fold; they decode nothing)
    uint64_t first_bad = ~0ull;
    for (uint64_t j = 0; j < dealt; ++j) {
        zi_pr_part part[MAX_LANES];
        bool ok = true;
        for (uint32_t l = 0; l < MAX_LANES; ++l) part[l] = zi_mpd_fold_run(mem[j], seg.data(), sums.data(), segok.data(), l, MAX_LANES, &ok);
        for (uint32_t o = 1; o < MAX_LANES; o <<= 1)
            for (uint32_t l = 0; l < MAX_LANES; ++l) zi_mpd_fold_step(part, l, MAX_LANES, o);
        if (!zi_mpd_verdict(src, n, mem[j], part[0], ok) && j < first_bad) first_bad = j;
    }
    const uint64_t f = first_bad < dealt ? first_bad : mstar;
    if (f == nmem) { stats[1] = nmem; *out_len = mem[nmem - 1].off + mem[nmem - 1].out; return ZI_ITEM_OK; }
    return tail(f, mem[f].c, mem[f].off);
}
