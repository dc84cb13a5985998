// inflate_harness.cpp -- CPU harness of the inflate core (zzflate_amd/csrc/zz_inflate_core.h), the same code the device
// decoder runs, with one lane. tests/test_inflate_core_cpu.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED
// (every buffer access of the core checked; out of range aborts the process) and calls it through ctypes.
//
//   zih_inflate  : a whole zlib / gzip / raw stream, serially (the serial path's run), container and checksum included
//   zih_packets  : the parallel paths' work done packet by packet -- phase 1 of every packet at its index offsets, then the
//                  pending bytes resolved by pointer-jumping rounds as the device does them -- and the same checks
#define HARNESS_NAME "inflate_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

uint32_t adler(const uint8_t* p, uint64_t n)
{
    uint32_t a = 1, b = 0;
    for (uint64_t i = 0; i < n; ++i) { a = (a + p[i]) % 65521; b = (b + a) % 65521; }
    return (b << 16) | a;
}
uint32_t crc(const uint8_t* p, uint64_t n)
{
    uint32_t c = ~0u;
    for (uint64_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * 0xEDB88320u); }
    return ~c;
}
int tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }

// 0 ok, -1 data, -2 no space, -5 preset dictionary (the ABI's codes)
int map_err(int e) { return e == ZI_E_SPACE ? -2 : -6; }

int check_trailer(int format, const uint8_t* t, const uint8_t* out, uint64_t n)
{
    if (format == 0) {
        const uint32_t want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
        return adler(out, n) == want ? 0 : -6;
    }
    if (format == 1) {
        const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        return (crc(out, n) == c && l == (uint32_t)n) ? 0 : -6;
    }
    return 0;
}

}  // namespace

extern "C" int zih_header(int format, const uint8_t* src, uint64_t n) { return (int)zi_header(format, src, n); }

extern "C" int zih_inflate(const uint8_t* src, uint64_t n, int format, uint8_t* out, uint64_t cap, uint64_t* out_len)
{
    *out_len = 0;
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return -5;
    if (hl < 0) return -6;
    std::vector<uint8_t> copy(src + hl, src + n);             // exactly the bytes behind the header: the checker sees overreads
    zi_view<const uint8_t> view{ copy.data(), copy.size() };
    host_in in{ view };
    zi_tables* S = new zi_tables();
    S->kind = 0;
    zi_out_linear<> o{ zi_view<uint8_t>{ out, cap }, 0, 0, 1, {} };
    const zi_result R = zi_run(in, view, 0, o, *S, ZI_RUN_STREAM, 0, 0, 1);
    delete S;
    if (R.err) return map_err(R.err);
    if (view.n - R.end != (uint64_t)tlen(format)) return -6;  // truncated trailer or bytes behind it
    *out_len = R.out;
    return check_trailer(format, copy.data() + R.end, out, R.out);
}

// index[0, entries) = packet starts relative to the first DEFLATE byte, index[entries-1] = the DEFLATE stream's end.
// stats[0] = pending bytes phase 1 left, stats[1] = pointer-jumping rounds, stats[2] = references in front of a packet start.
extern "C" int zih_packets(const uint8_t* src, uint64_t n, int format, uint32_t P, const uint64_t* index, uint64_t entries,
                           uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* stats)
{
    *out_len = 0;
    stats[0] = stats[1] = stats[2] = 0;
    const int64_t hl = zi_header(format, src, n);
    if (hl < 0 || entries < 2 || P == 0) return -6;
    const uint64_t npk = entries - 1;
    const uint64_t sbytes = n - (uint64_t)hl;
    if (index[0] != 0 || index[npk] + tlen(format) != sbytes) return -6;
    const uint64_t total_max = npk * P;
    std::vector<uint8_t> dst(total_max);
    std::vector<uint32_t> st(total_max, 0);                    // one batch: the whole call
    std::vector<uint32_t> pend(npk * ((P + 31) / 32), 0);
    std::vector<uint32_t> pcnt(npk, 0);
    uint64_t total = 0;
    zi_tables* S = new zi_tables();
    for (uint64_t k = 0; k < npk; ++k) {
        if (index[k + 1] <= index[k] || index[k + 1] > sbytes) { delete S; return -6; }
        std::vector<uint8_t> pk(src + hl + index[k], src + hl + index[k + 1]);   // the packet alone
        zi_view<const uint8_t> view{ pk.data(), pk.size() };
        host_in in{ view };
        S->kind = 0;
        std::vector<uint8_t> win(P);
        zi_out_packet<zi_fence_none, zi_or_plain> o{ zi_view<uint8_t>{ win.data(), P },
                                                     zi_view<uint32_t>{ pend.data() + k * ((P + 31) / 32), (P + 31) / 32 },
                                                     zi_view<uint32_t>{ st.data() + k * P, P },
                                                     k * P, (int64_t)(k * P), 0, 0, false, 0, 1, {}, {} };
        const zi_result R = zi_run(in, view, 0, o, *S, ZI_RUN_INDEXED, P, 0, 1);
        const bool last = k + 1 == npk;
        if (R.err || (R.final != 0) != last || (last && R.end != view.n)) { delete S; return -6; }
        memcpy(dst.data() + k * P, win.data(), R.out);
        pcnt[k] = o.npend;
        stats[0] += o.npend;
        if (o.npend) stats[2]++;
        total = k * P + R.out;
    }
    delete S;
    // pointer jumping, as the device's rounds: a round reads the state the previous one left
    std::vector<uint32_t> nst = st;
    std::vector<uint8_t> done_round(total_max, 0);             // round in which a pending byte became final (0: not yet)
    auto pending = [&](uint64_t x) { return pcnt[x / P] && ((pend[(x / P) * ((P + 31) / 32) + (x % P) / 32] >> ((x % P) & 31)) & 1u); };
    for (uint32_t round = 1;; ++round) {
        uint64_t left = 0;
        for (uint64_t x = 0; x < total; ++x) {
            if (!pending(x) || done_round[x]) continue;
            const int64_t t = (int64_t)(st[x] & ZI_PTR_MASK) - (int64_t)ZI_BIAS;
            if (t < 0) return -6;                              // in front of the stream: phase 1 refuses these
            const uint64_t y = (uint64_t)t;
            if (!pending(y) || (done_round[y] && done_round[y] < round)) { dst[x] = dst[y]; done_round[x] = (uint8_t)round; }
            else { nst[x] = st[y]; ++left; }
        }
        st = nst;
        if (left == 0) { stats[1] = stats[0] ? round : 0; break; }
        if (round > 40) return -6;
    }
    if (total > cap) return -2;
    memcpy(out, dst.data(), total);
    *out_len = total;
    return check_trailer(format, src + n - tlen(format), out, total);
}
