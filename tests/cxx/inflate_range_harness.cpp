// inflate_range_harness.cpp -- CPU harness of the range decode (zz_decode_range_device): bytes [first, first + n) of an indexed
// packet-mode stream, by the procedure the device runs and with the rules it shares through zz_inflate_core.h -- phase 1 from
// packet kb = k0 - h with pointers relative to kb * P, the pointer-jumping rounds with external pointers, the bytes carried
// from one batch into the next, the growth of the look-back. tests/test_inflate_range_cpu.py builds it with g++
// -fsanitize=undefined -DZZ_INFLATE_CHECKED and calls it through ctypes.
//
//   zrh_range : one call; `batch_packets` (0: the device's batch) lets a test send a few KiB through several batches
#define HARNESS_NAME "inflate_range_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

int tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }

struct attempt_result { int rc; uint64_t ext, pending, L; bool saw_last; };

// packets [kb, k1) in batches of B; the window's bytes go to res[0, ..) (res holds (k1 - k0) * P bytes)
attempt_result attempt(const uint8_t* s, uint64_t sn, const uint64_t* index, uint64_t npk, uint32_t P, uint64_t kb, uint64_t k1,
                       uint64_t B, uint64_t first, uint64_t nbytes, std::vector<uint8_t>& res)
{
    attempt_result A{ 0, 0, 0, 0, false };
    const uint32_t words = (P + 31) / 32;
    if (B > k1 - kb) B = k1 - kb;
    std::vector<uint8_t> stage(ZI_BIAS + B * P, 0);
    std::vector<uint32_t> carry(ZI_BIAS / 32, ~0u);              // the first batch: everything below it is external
    std::vector<uint32_t> st(B * P), pend(B * words), pcnt(B);
    zi_tables* S = new zi_tables();
    for (uint64_t kf = kb; kf < k1; kf += B) {
        const uint64_t nb = k1 - kf < B ? k1 - kf : B;
        const uint64_t base = kf * P;                            // absolute position of the batch's first byte
        zi_view<uint8_t> sg{ stage.data(), stage.size() };      // the carried bytes, then the batch's
        zi_view<uint8_t> area{ stage.data() + ZI_BIAS, nb * P };
        std::fill(pend.begin(), pend.end(), 0u);
        uint64_t produced = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t k = kf + b;
            if (index[k + 1] <= index[k] || index[k + 1] > sn) { delete S; A.rc = -6; return A; }
            std::vector<uint8_t> pk(s + index[k], s + index[k + 1]);            // the packet alone: the checker sees overreads
            zi_view<const uint8_t> view{ pk.data(), pk.size() };
            host_in in{ view };
            S->kind = 0;
            zi_out_packet<zi_fence_none, zi_or_plain> o{ zi_view<uint8_t>{ area.p + b * P, P }, zi_view<uint32_t>{ pend.data() + b * words, words },
                                                         zi_view<uint32_t>{ st.data() + b * P, P },
                                                         k * P, (int64_t)(b * P), 0, 0, false, 0, 1, {}, {} };
            const zi_result R = zi_run(in, view, 0, o, *S, ZI_RUN_INDEXED, P, 0, 1);
            const bool last = k + 1 == npk;
            if (R.err || (R.final != 0) != last || (last && R.end != view.n)) { delete S; A.rc = -6; return A; }
            pcnt[b] = o.npend;
            A.pending += o.npend;
            produced = b * P + R.out;
            if (last) { A.saw_last = true; A.L = k * P + R.out; }
        }
        // the rounds, in place and in order of position: one of the orders the device's lanes may take
        const zi_view<const uint32_t> cv{ carry.data(), carry.size() };
        zi_view<uint32_t> sv{ st.data(), nb * P };
        auto pending = [&](uint64_t x) { return pcnt[x / P] && ((pend[(x / P) * words + (x % P) / 32] >> ((x % P) & 31)) & 1u); };
        for (uint32_t round = 1;; ++round) {
            uint64_t left = 0;
            for (uint64_t x = 0; x < produced; ++x) {
                if (!pending(x)) continue;
                const uint32_t w = sv[x];
                if (w >> 27) continue;
                const int64_t y = (int64_t)(w & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
                bool fin = false, ext = false;
                if (y < 0) { ext = zi_range_external(y, cv); fin = !ext; }
                else if (!pending((uint64_t)y)) fin = true;
                else {
                    const uint32_t wy = sv[(uint64_t)y], ry = wy >> 27;
                    if (ry == ZI_ROUND_EXTERNAL) ext = true;
                    else if (ry != 0 && ry < round) fin = true;
                    else { sv[x] = wy & ZI_PTR_MASK; ++left; }
                }
                if (fin) {
                    ZI_CHECK(y < (int64_t)x);
                    area[x] = sg[(uint64_t)((int64_t)ZI_BIAS + y)];
                    sv[x] = (w & ZI_PTR_MASK) | (round << 27);
                }
                if (ext) {
                    sv[x] = (w & ZI_PTR_MASK) | (ZI_ROUND_EXTERNAL << 27);
                    const uint64_t a = base + x;
                    if (a >= first && a - first < nbytes) ++A.ext;
                }
            }
            if (left == 0) break;
            if (round >= 30) { delete S; A.rc = -6; return A; }
        }
        // the window's part of this batch
        for (uint64_t x = 0; x < produced; ++x) {
            const uint64_t a = base + x;
            if (a >= first && a - first < nbytes) res[a - first] = area[x];
        }
        // what the next batch may point at: the last ZI_BIAS bytes and whether they are external
        if (kf + nb < k1) {
            ZI_CHECK(nb * P >= ZI_BIAS);
            std::vector<uint32_t> nc(ZI_BIAS / 32, 0u);
            for (uint64_t i = 0; i < ZI_BIAS; ++i) {
                const uint64_t x = nb * P - ZI_BIAS + i;
                stage[i] = area[x];
                if (pending(x) && (sv[x] >> 27) == ZI_ROUND_EXTERNAL) nc[i >> 5] |= 1u << (i & 31);
            }
            carry = nc;
        }
    }
    delete S;
    return A;
}

}  // namespace

extern "C" uint64_t zrh_first_lookback(uint32_t P, uint64_t k0) { return zi_range_first_lookback(P, k0); }
extern "C" uint64_t zrh_next_lookback(uint64_t h, uint64_t k0) { return zi_range_next_lookback(h, k0); }

// The ABI's codes: 0 ok, -2 no space, -4 argument, -5 preset dictionary, -6 data.
// stats[0] = first packet decoded, [1] = packets of the final attempt, [2] = attempts, [3] = pending bytes of the final attempt
extern "C" int zrh_range(const uint8_t* src, uint64_t n, int format, uint32_t P, const uint64_t* index, uint64_t entries,
                         uint64_t first, uint64_t nbytes, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* stats,
                         uint64_t batch_packets)
{
    if (!src || !index || !out_len) return -4;
    *out_len = 0;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (P < 1 || P > 32768 || format < 0 || format > 2 || entries < 2) return -4;
    const uint64_t npk = entries - 1;
    if (first / P >= npk || first + nbytes < first) return -4;
    if (nbytes == 0) return 0;
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return -5;
    if (hl < 0 || n < (uint64_t)hl + tlen(format)) return -6;
    const uint8_t* s = src + hl;
    const uint64_t sn = n - (uint64_t)hl - tlen(format);
    if (index[0] != 0 || index[npk] != sn) return -6;
    const uint64_t k0 = first / P;
    const uint64_t lastk = (first + nbytes - 1) / P;
    const uint64_t k1 = lastk + 1 < npk ? lastk + 1 : npk;
    uint64_t B = batch_packets;
    if (B == 0) { B = (64ull << 20) / P; if (B > (1u << 18)) B = 1u << 18; }
    std::vector<uint8_t> res((k1 - k0) * P);
    uint64_t h = zi_range_first_lookback(P, k0);
    for (uint32_t tries = 1;; ++tries) {
        const uint64_t kb = k0 - h;
        const attempt_result A = attempt(s, sn, index, npk, P, kb, k1, B, first, nbytes, res);
        if (A.rc) return A.rc;
        stats[0] = kb; stats[1] = k1 - kb; stats[2] = tries; stats[3] = A.pending;
        if (A.ext != 0) {
            if (kb == 0) return -6;                                // (phase 1 refuses what would point in front of the stream)
            h = zi_range_next_lookback(h, k0);
            continue;
        }
        uint64_t m = nbytes;
        if (A.saw_last) { const uint64_t rest = A.L > first ? A.L - first : 0; if (m > rest) m = rest; }
        if (m > cap) { *out_len = ~0ull; return -2; }
        if (m) memcpy(out, res.data(), m);
        *out_len = m;
        return 0;
    }
}
