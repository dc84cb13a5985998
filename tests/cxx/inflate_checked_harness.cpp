// inflate_checked_harness.cpp -- CPU harness of the checked range read (zz_decode_range_checked_device): the range decode's
// procedure as tests/cxx/inflate_range_harness.cpp runs it, with the packet checksum sidecar's rules from zz_inflate_core.h on
// top -- the sidecar unpacked and folded against the stream's trailer before anything is decoded, the widened window inside
// which an external byte sends the read back, every touched packet summed on the stage (its length from phase 1) and held to
// its entry. tests/test_checked_cases_cpu.py builds it with g++ -fsanitize=undefined -DZZ_INFLATE_CHECKED and calls it through
// ctypes.
//
//   zch_range   : one call; cks == NULL is the unchecked read. `batch_packets` (0: the device's batch) sends a few KiB through
//                 several batches; `lanes` (1 or 64) is how many lanes share a packet's sum, each with the device's share of it
//   zch_sidecar : the sidecar of a buffer, by the same lane sums and zi_cks_public
#define HARNESS_NAME "inflate_checked_harness"
#include "harness_lanes.h"

using namespace zz;

namespace {

int tlen(int format) { return format == 0 ? 4 : format == 1 ? 8 : 0; }

// a packet's start-0 partial by `nl` lanes. Adler: lane l takes the 16-byte chunks l, l + nl, ... and the byte l behind the last
// whole chunk (wave_adler's shares), raw sums A = sum d, C = sum i * d, then a = A, b = len * A - C. CRC: lane l takes a contiguous
// slice and shifts its CRC over the bytes behind it (the checksum kernel's plain path).
void packet_partial(int kind, const zi_view<const uint8_t>& p, uint32_t len, uint32_t nl, uint32_t* a, uint32_t* b)
{
    if (kind == ZI_CKS_ADLER) {
        uint64_t At = 0, Ct = 0;
        const uint32_t nchunks = len >> 4;
        for (uint32_t l = 0; l < nl; ++l) {
            uint64_t A = 0, C = 0;
            for (uint32_t c = l; c < nchunks; c += nl)
                for (uint32_t j = 0; j < 16; ++j) { const uint64_t i = ((uint64_t)c << 4) + j; A += p[i]; C += i * p[i]; }
            for (uint32_t i = (nchunks << 4) + l; i < len; i += nl) { A += p[i]; C += (uint64_t)i * p[i]; }
            At += A; Ct += C;
        }
        *a = (uint32_t)(At % ZZ_ADLER_MOD);
        *b = (uint32_t)(((uint64_t)len * At - Ct) % ZZ_ADLER_MOD);
        return;
    }
    uint32_t r = 0;
    const uint32_t slice = ((len + nl - 1) / nl + 3) & ~3u;
    for (uint32_t l = 0; l < nl; ++l) {
        uint32_t b0 = l * slice, b1 = b0 + slice;
        if (b0 > len) b0 = len;
        if (b1 > len) b1 = len;
        if (b1 <= b0) continue;
        uint32_t c = ~0u;
        for (uint32_t i = b0; i < b1; ++i) {
            c ^= p[i];
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * ZZ_CRC_POLY);
        }
        r ^= gf2_mulmod(~c, gf2_xpow8(len - b1));
    }
    *a = r; *b = 0;
}

// the sidecar against the trailer: unpack, fold in packet order, verdict
bool sidecar_holds(int format, const uint8_t* trailer, const uint32_t* cks, uint64_t npk, uint32_t P, uint64_t L)
{
    if (format == 2) return true;
    const int kind = zi_sidecar_kind(format);
    uint32_t fold = 0;                                           // Adler: (b << 16) | a of the bytes so far, start value 0
    zi_view<const uint32_t> cv{ cks, npk };
    for (uint64_t k = 0; k < npk; ++k) {
        const uint32_t len = zi_sidecar_len(k, L, P);
        uint32_t a = 0, b = 0;
        if (!zi_cks_partial(kind, cv[k], len, &a, &b)) return false;
        fold = kind == ZI_CKS_ADLER ? adler_combine(fold, (b << 16) | a, len) : crc32_combine(fold, a, len);
    }
    return zi_sidecar_trailer_ok(format, trailer, kind == ZI_CKS_ADLER ? fold & 0xFFFFu : fold, kind == ZI_CKS_ADLER ? fold >> 16 : 0u, L);
}

struct attempt_result { int rc; uint64_t ext, pending, L, bad; bool saw_last; };
struct sidecar { const uint32_t* cks; uint64_t L; int kind; uint32_t lanes; };

// packets [kb, k1) in batches of B; the window's bytes go to res[0, ..) (res holds (k1 - k0) * P bytes)
attempt_result attempt(const uint8_t* s, uint64_t sn, const uint64_t* index, uint64_t npk, uint32_t P, uint64_t kb, uint64_t k1,
                       uint64_t B, uint64_t first, uint64_t nbytes, const sidecar& sc, std::vector<uint8_t>& res)
{
    attempt_result A{ 0, 0, 0, 0, 0, false };
    const uint32_t words = (P + 31) / 32;
    const uint64_t k0 = first / P;
    if (B > k1 - kb) B = k1 - kb;
    std::vector<uint8_t> stage(ZI_BIAS + B * P, 0);
    std::vector<uint32_t> carry(ZI_BIAS / 32, ~0u);              // the first batch: everything below it is external
    std::vector<uint32_t> st(B * P), pend(B * words), pcnt(B), outb(B);
    uint64_t xlo = 0, xhi = 0;
    zi_checked_window(sc.cks != nullptr, first, nbytes, P, k0, k1, &xlo, &xhi);
    zi_view<const uint32_t> cv{ sc.cks, sc.cks ? npk : 0 };
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
            outb[b] = (uint32_t)R.out;
            A.pending += o.npend;
            produced = b * P + R.out;
            if (last) { A.saw_last = true; A.L = k * P + R.out; }
        }
        // the rounds, in place and in order of position: one of the orders the device's lanes may take
        const zi_view<const uint32_t> cvx{ carry.data(), carry.size() };
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
                if (y < 0) { ext = zi_range_external(y, cvx); fin = !ext; }
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
                    if (a >= xlo && a < xhi) ++A.ext;
                }
            }
            if (left == 0) break;
            if (round >= 30) { delete S; A.rc = -6; return A; }
        }
        // the batch's touched packets against the sidecar: lengths from phase 1
        if (sc.cks) {
            for (uint64_t b = 0; b < nb; ++b) {
                const uint64_t k = kf + b;
                if (k < k0) continue;
                uint32_t pa = 0, pb = 0;
                packet_partial(sc.kind, zi_view<const uint8_t>{ area.p + b * P, outb[b] }, outb[b], sc.lanes, &pa, &pb);
                if (zi_checked_packet_bad(sc.kind, pa, pb, outb[b], cv[k], k, npk, sc.L, P)) ++A.bad;
            }
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

extern "C" uint32_t zch_public(int kind, uint32_t a, uint32_t b, uint32_t len) { return zi_cks_public(kind, a, b, len); }
extern "C" int zch_partial(int kind, uint32_t v, uint32_t len, uint32_t* a, uint32_t* b) { return zi_cks_partial(kind, v, len, a, b) ? 1 : 0; }
extern "C" uint64_t zch_entries(uint64_t L, uint32_t P) { return zi_sidecar_entries(L, P); }

// the sidecar of data[0, n): out holds zch_entries(n, P) values
extern "C" void zch_sidecar(const uint8_t* data, uint64_t n, int format, uint32_t P, uint32_t lanes, uint32_t* out)
{
    const int kind = zi_sidecar_kind(format);
    const uint64_t npk = zi_sidecar_entries(n, P);
    zi_view<uint32_t> ov{ out, npk };
    for (uint64_t k = 0; k < npk; ++k) {
        const uint32_t len = zi_sidecar_len(k, n, P);
        uint32_t a = 0, b = 0;
        packet_partial(kind, zi_view<const uint8_t>{ data + k * P, len }, len, lanes, &a, &b);
        ov[k] = zi_cks_public(kind, a, b, len);
    }
}

// The ABI's codes: 0 ok, -2 no space, -4 argument, -5 preset dictionary, -6 data.
// stats[0] = first packet decoded, [1] = packets of the final attempt, [2] = attempts, [3] = pending bytes of the final attempt
extern "C" int zch_range(const uint8_t* src, uint64_t n, int format, uint32_t P, const uint64_t* index, uint64_t entries,
                         const uint32_t* cks, uint64_t total_len, uint64_t first, uint64_t nbytes, uint8_t* out, uint64_t cap,
                         uint64_t* out_len, uint64_t* stats, uint64_t batch_packets, uint32_t lanes)
{
    if (!src || !index || !out_len) return -4;
    *out_len = 0;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (P < 1 || P > 32768 || format < 0 || format > 2 || entries < 2 || lanes < 1 || lanes > 64) return -4;
    const uint64_t npk = entries - 1;
    if (first / P >= npk || first + nbytes < first) return -4;
    if (cks && (npk > 0x7fffffffull || npk != zi_sidecar_entries(total_len, P))) return -4;
    if (nbytes == 0) return 0;
    const int64_t hl = zi_header(format, src, n);
    if (hl == -2) return -5;
    if (hl < 0 || n < (uint64_t)hl + tlen(format)) return -6;
    const uint8_t* s = src + hl;
    const uint64_t sn = n - (uint64_t)hl - tlen(format);
    if (index[0] != 0 || index[npk] != sn) return -6;
    if (cks && !sidecar_holds(format, s + sn, cks, npk, P, total_len)) { *out_len = ~0ull; return -6; }
    const sidecar sc{ cks, total_len, zi_sidecar_kind(format), lanes };
    const uint64_t k0 = first / P;
    const uint64_t lastk = (first + nbytes - 1) / P;
    const uint64_t k1 = lastk + 1 < npk ? lastk + 1 : npk;
    uint64_t B = batch_packets;
    if (B == 0) { B = (64ull << 20) / P; if (B > (1u << 18)) B = 1u << 18; }
    std::vector<uint8_t> res((k1 - k0) * P);
    uint64_t h = zi_range_first_lookback(P, k0);
    for (uint32_t tries = 1;; ++tries) {
        const uint64_t kb = k0 - h;
        const attempt_result A = attempt(s, sn, index, npk, P, kb, k1, B, first, nbytes, sc, res);
        if (A.rc) { if (cks && A.rc == -6) *out_len = ~0ull; return A.rc; }
        stats[0] = kb; stats[1] = k1 - kb; stats[2] = tries; stats[3] = A.pending;
        if (A.ext != 0) {
            if (kb == 0) return -6;                                // (phase 1 refuses what would point in front of the stream)
            h = zi_range_next_lookback(h, k0);
            continue;
        }
        if (A.bad != 0) { *out_len = ~0ull; return -6; }
        uint64_t m = nbytes;
        if (A.saw_last) { const uint64_t rest = A.L > first ? A.L - first : 0; if (m > rest) m = rest; }
        if (m > cap) { *out_len = ~0ull; return -2; }
        if (m) memcpy(out, res.data(), m);
        *out_len = m;
        return 0;
    }
}
