// inflate_ranges_harness.cpp -- CPU harness of the multi-range decode (zz_decode_ranges_device): many reads of one indexed
// packet-mode stream in one call, by the procedure the device runs and with the rules it shares through zz_inflate_core.h -- the
// plan (zi_ranges_plan, an exclusive scan of segment lengths), the waves (zi_ranges_wave), one descriptor per stage packet
// (zi_ranges_desc), phase 1 with pointers relative to the segment, the rounds in which a target below the segment's base is
// external, the verdict (zi_ranges_verdict) and the copy. tests/test_inflate_ranges_cpu.py builds it with g++
// -fsanitize=undefined -DZZ_INFLATE_CHECKED and calls it through ctypes.
//
//   zrs_ranges : one call; `wave_packets` (0: the device's batch) and `limit_packets` (0: the device's batch) let a test send a
//                few reads through several waves and meet the per-read limit with a few KiB
#define HARNESS_NAME "inflate_ranges_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

int tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }
uint32_t ceil_log2(uint64_t x) { uint32_t r = 0; while ((1ull << r) < x) ++r; return r; }

}  // namespace

// The ABI's codes: 0 ok, -2 no space, -4 argument, -5 unsupported, -6 data; -100: the harness's own (rounds did not suffice).
// stats[0] = stage packets over all attempts, [1] = attempts, [2] = reads with more than one attempt, [3] = waves
extern "C" int zrs_ranges(const uint8_t* src, uint64_t n, int format, uint32_t P, const uint64_t* index, uint64_t entries,
                          uint64_t nranges, const uint64_t* firsts, const uint64_t* nbytes, uint8_t* const* dsts, const uint64_t* caps,
                          uint64_t* out_lens, int32_t* status, uint64_t* stats, uint64_t wave_packets, uint64_t limit_packets)
{
    if (!src || !index || !firsts || !nbytes || !dsts || !caps || !out_lens) return -4;
    if (P < 1 || P > 32768 || format < 0 || format > 2 || entries < 2 || nranges > 0x7fffffffull) return -4;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (nranges == 0) return 0;
    const uint64_t npk = entries - 1;
    auto fail_all = [&](int code) { for (uint64_t r = 0; r < nranges; ++r) { out_lens[r] = ~0ull; if (status) status[r] = code; } return code; };
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return fail_all(-5);
    if (hl < 0 || n < (uint64_t)hl + tlen(format)) return fail_all(-6);
    const uint8_t* s = src + hl;
    const uint64_t sn = n - (uint64_t)hl - tlen(format);
    if (index[0] != 0 || index[npk] != sn) return fail_all(-6);
    uint64_t B = (64ull << 20) / P;
    if (B > (1u << 18)) B = 1u << 18;
    const uint64_t W = wave_packets ? wave_packets : B, limit = limit_packets ? limit_packets : B;
    const uint32_t words = (P + 31) / 32;

    std::vector<zi_read> reads(nranges, zi_read{ 0, 0, 0, 0, ZI_RS_NEW, 0, 0, 0, 0 });
    uint64_t count[7] = { 0, 0, 0, 0, 0, 0, 0 };                 // settled reads by -status
    auto settle = [&](uint64_t r) {
        out_lens[r] = reads[r].status == ZI_RV_OK ? reads[r].m : ~0ull;
        if (status) status[r] = reads[r].status;
        ++count[-reads[r].status];
    };
    zi_tables* S = new zi_tables();
    int harness_rc = 0;
    for (uint32_t tries = 1; !harness_rc; ++tries) {
        // the plan: segment lengths, their exclusive scan, the longest
        uint64_t base = 0, longest = 0;
        for (uint64_t r = 0; r < nranges; ++r) {
            const bool open = reads[r].state != ZI_RS_DONE;
            const uint64_t l = zi_ranges_plan(reads[r], firsts[r], nbytes[r], P, npk, limit);
            reads[r].npk = (uint32_t)l; reads[r].base = base;
            if (open && reads[r].state == ZI_RS_DONE) settle(r);
            base += l;
            if (l > longest) longest = l;
        }
        if (base == 0) break;
        stats[0] += base; stats[1] = tries;
        const uint32_t rounds = ceil_log2(longest) + 2;
        // the waves: runs of reads whose segments start in the same [w * W, (w + 1) * W)
        uint64_t r = 0;
        while (r < nranges) {
            while (r < nranges && reads[r].npk == 0) ++r;
            if (r == nranges) break;
            const uint64_t w = zi_ranges_wave(reads[r].base, W), g0 = reads[r].base, rlo = r;
            while (r < nranges && (reads[r].npk == 0 || zi_ranges_wave(reads[r].base, W) == w)) ++r;
            const uint64_t rhi = r;
            uint64_t g1 = g0;
            for (uint64_t q = rlo; q < rhi; ++q) if (reads[q].npk) g1 = reads[q].base + reads[q].npk;
            const uint64_t nb = g1 - g0;
            ++stats[3];
            std::vector<uint8_t> stage(nb * P, 0);
            std::vector<uint32_t> st(nb * P), pend(nb * words, 0u), pcnt(nb, 0u), stat(nb, 0u);
            std::vector<zi_read_desc> desc(nb);
            for (uint64_t q = rlo; q < rhi; ++q)
                for (uint64_t j = 0; j < reads[q].npk; ++j)
                    desc[reads[q].base - g0 + j] = zi_ranges_desc(reads[q], (uint32_t)q, j, (uint32_t)(reads[q].base - g0), firsts[q], nbytes[q], P);
            // phase 1
            for (uint64_t b = 0; b < nb; ++b) {
                const zi_read_desc& D = desc[b];
                const uint64_t k = D.k;
                ZI_CHECK(k < npk && D.seg0 <= b);
                bool ok = index[k + 1] > index[k] && index[k + 1] <= sn;
                zi_result R{ ZI_E_DATA, 0, 0, 0 };
                uint32_t np = 0;
                if (ok) {
                    std::vector<uint8_t> pk(s + index[k], s + index[k + 1]);            // the packet alone: the checker sees overreads
                    zi_view<const uint8_t> view{ pk.data(), pk.size() };
                    host_in in{ view };
                    S->kind = 0;
                    zi_out_packet<zi_fence_none, zi_or_plain> o{ zi_view<uint8_t>{ stage.data() + b * P, P }, zi_view<uint32_t>{ pend.data() + b * words, words },
                                                                 zi_view<uint32_t>{ st.data() + b * P, P },
                                                                 k * P, (int64_t)((b - D.seg0) * P), 0, 0, false, 0, 1, {}, {} };
                    R = zi_run(in, view, 0, o, *S, ZI_RUN_INDEXED, P, 0, 1);
                    np = o.npend;
                    const bool last = k + 1 == npk;
                    if (!R.err && ((R.final != 0) != last || (last && R.end != view.n))) R.err = ZI_E_SHAPE;
                }
                pcnt[b] = R.err ? 0u : np;
                stat[b] = R.err ? 0u : (1u | ((uint32_t)R.out << 3));
                if (R.err) ++reads[D.read].fail;
            }
            // the rounds, in place and in order of position: one of the orders the device's lanes may take
            zi_view<uint32_t> sv{ st.data(), st.size() };
            zi_view<uint8_t> sg{ stage.data(), stage.size() };
            auto pending = [&](uint64_t x) { return pcnt[x / P] && ((pend[(x / P) * words + (x % P) / 32] >> ((x % P) & 31)) & 1u); };
            uint64_t left = 0;
            for (uint32_t round = 1; round <= rounds; ++round) {
                left = 0;
                for (uint64_t x = 0; x < nb * P; ++x) {
                    if (!pending(x)) continue;
                    const zi_read_desc& D = desc[x / P];
                    const uint64_t sb = (uint64_t)D.seg0 * P;
                    const uint32_t q = (uint32_t)(x % P);
                    const uint32_t wd = sv[x];
                    if (wd >> 27) continue;
                    const int64_t y = (int64_t)(wd & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
                    bool fin = false, ext = false;
                    if (y < 0) ext = true;                                             // below the segment's base
                    else if (!pending(sb + (uint64_t)y)) fin = true;
                    else {
                        const uint32_t wy = sv[sb + (uint64_t)y], ry = wy >> 27;
                        if (ry == ZI_ROUND_EXTERNAL) ext = true;
                        else if (ry != 0 && ry < round) fin = true;
                        else { sv[x] = wy & ZI_PTR_MASK; ++left; }
                    }
                    if (fin) {
                        ZI_CHECK(sb + (uint64_t)y < x);
                        sg[x] = sg[sb + (uint64_t)y];
                        sv[x] = (wd & ZI_PTR_MASK) | (round << 27);
                    }
                    if (ext) {
                        sv[x] = (wd & ZI_PTR_MASK) | (ZI_ROUND_EXTERNAL << 27);
                        if (q >= D.lo && q < D.hi) ++reads[D.read].ext;
                    }
                }
            }
            if (left) { harness_rc = -100; break; }                                    // ceil(log2(longest)) + 2 rounds must suffice
            // the verdict per read, then the copy per stage packet
            for (uint64_t q = rlo; q < rhi; ++q) {
                if (reads[q].npk == 0) continue;
                const uint32_t before = reads[q].tries;
                const uint32_t last_out = stat[reads[q].base - g0 + reads[q].npk - 1] >> 3;
                const int v = zi_ranges_verdict(reads[q], firsts[q], nbytes[q], caps[q], P, npk, limit, last_out);
                if (v == ZI_RV_AGAIN && before == 0) ++stats[2];
                if (v != ZI_RV_AGAIN) settle(q);
            }
            for (uint64_t b = 0; b < nb; ++b) {
                const zi_read_desc& D = desc[b];
                const zi_read& R = reads[D.read];
                if (R.state != ZI_RS_DONE || R.status != ZI_RV_OK) continue;
                const uint64_t first = firsts[D.read], a = D.k * P + D.lo;
                uint64_t e = D.k * P + D.hi;
                if (e > first + R.m) e = first + R.m;
                if (e <= a) continue;
                ZI_CHECK(a >= first && e - first <= caps[D.read]);
                memcpy(dsts[D.read] + (a - first), stage.data() + b * P + D.lo, e - a);
            }
        }
    }
    delete S;
    if (harness_rc) return harness_rc;
    if (count[6]) return -6;
    if (count[5]) return -5;
    if (count[4]) return -4;
    if (count[2]) return -2;
    return 0;
}
