// zz_inflate_core.h -- the RFC 1951 inflate core shared by the device decoder (zz_inflate.h) and its CPU harness
// (tests/cxx/inflate_harness.cpp): bit reader, block headers, code-length parsing, canonical table construction,
// symbol decode and every bounds check live here, once -- and, for the batch decoder (k_inflate_items) and its harness
// (tests/cxx/inflate_items_harness.cpp), zi_item: one complete stream, container header to checksum, by one group of lanes.
//
// The core is written for a group of `nl` lanes that run the same control flow (one wavefront on the device, one
// thread on the host): every lane decodes every symbol (the bit reader, the tables and the block state are uniform),
// and only the writes are divided -- table fills, stored bytes and match copies are lane-strided. Compiles with g++
// without HIP (ZZ_HD is empty there); with -DZZ_INFLATE_CHECKED every buffer access goes through ZI_CHECK, which aborts
// on an index out of range, so that a CPU build proves the bounds the device relies on.
//
// Tables: a 10-bit first level plus second-level tables for longer codes, 16-bit entries:
//   bit 15 = 0 : bits 0..8 symbol (0x1FF: no code), bits 9..12 bits to consume (0: no code)
//   bit 15 = 1 : link; bits 0..10 = index of the second-level table, bits 11..14 = its index bits
// zlib's `enough` bounds a 286-symbol, root-10, 15-bit code at 1332 entries and a 30-symbol one well below that;
// ZI_TAB leaves room, and the builder still refuses (as invalid) a code that would not fit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define ZZ_HD __host__ __device__
#else
#define ZZ_HD
#endif

#ifdef ZZ_INFLATE_CHECKED
#include <cstdio>
#include <cstdlib>
#define ZI_CHECK(c) do { if (!(c)) { fprintf(stderr, "zz_inflate_core: access out of range at line %d\n", __LINE__); abort(); } } while (0)
#else
#define ZI_CHECK(c) ((void)0)
#endif

// The lanes of a wavefront run in lockstep, so what one lane writes to a table is there when another lane reads it an
// instruction later: on the device this is nothing. A CPU harness that runs the lanes one after the other defines it as
// "let every other lane get here" (tests/cxx/inflate_items_harness.cpp).
#ifndef ZI_LANES_SYNC
#define ZI_LANES_SYNC() ((void)0)
#endif

namespace zz {

// results of the core (the C ABI maps them: DATA / FAR -> ZZ_E_DATA, SPACE -> ZZ_E_NOSPACE)
enum { ZI_OK = 0, ZI_E_DATA = 1, ZI_E_SPACE = 2, ZI_E_FAR = 3, ZI_E_SHAPE = 4,
       ZI_E_GAVEUP = 5 };      // ZI_RUN_REACH only: the run passed its `limit` bit in mid-block (zi_pt_reach)

#define ZI_ROOT 10
#define ZI_TAB 1536
#define ZI_NOCODE 0x01FFu

// a bounds-checked window onto a buffer (checked only in ZZ_INFLATE_CHECKED builds)
template <class T> struct zi_view {
    T* p; uint64_t n;
    ZZ_HD T& operator[](uint64_t i) const { ZI_CHECK(i < n); return p[i]; }
};

// table memory of one decoder (LDS on the device): 2 * 3 KiB + scratch
struct zi_tables {
    uint16_t lit[ZI_TAB];
    uint16_t dst[ZI_TAB];
    uint16_t sorted[320];       // symbols in canonical order
    uint8_t lens[320];          // code lengths of the block being read (litlen followed by distance)
    uint16_t cnt[16], offs[16];
    int kind;                   // what `lit`/`dst` hold now: 0 nothing, 1 the fixed code, 2 a dynamic code
};

ZZ_HD inline uint32_t zi_rev(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

// Canonical code (RFC 1951 3.2.2) from lens[0, n) into tab. Validity as zlib: over-subscribed codes are refused;
// incomplete codes only in the form of a single one-bit code (literal/length and distance codes; the unused half of
// the table stays "no code") -- `allow_empty` additionally accepts no code at all (a block without distances). Lanes split the fills; the serial parts are done by every lane alike.
ZZ_HD inline bool zi_build(zi_view<uint16_t> tab, zi_tables& S, int n, bool allow_empty, bool allow_incomplete,
                           uint32_t lane, uint32_t nl)
{
    zi_view<uint8_t> lens{ S.lens, 320 };
    zi_view<uint16_t> cnt{ S.cnt, 16 }, offs{ S.offs, 16 }, sorted{ S.sorted, 320 };
    ZI_LANES_SYNC();                                        // every lane has finished with what `tab` held
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int i = 0; i < n; ++i) cnt[lens[i]] = (uint16_t)(cnt[lens[i]] + 1);
    int maxl = 0;
    for (int l = 1; l < 16; ++l) if (cnt[l]) maxl = l;
    for (uint32_t i = lane; i < ZI_TAB; i += nl) tab[i] = (uint16_t)ZI_NOCODE;
    ZI_LANES_SYNC();                                        // the fills below land on entries other lanes cleared
    if (maxl == 0) return allow_empty;
    int left = 1;
    for (int l = 1; l < 16; ++l) { left = (left << 1) - cnt[l]; if (left < 0) return false; }
    if (left > 0 && !(allow_incomplete && maxl == 1)) return false;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (int i = 0; i < n; ++i) if (lens[i]) { sorted[offs[lens[i]]] = (uint16_t)i; offs[lens[i]] = (uint16_t)(offs[lens[i]] + 1); }
    // walk the codes in canonical order; codes longer than the root share second-level tables per root prefix. The
    // codes under one prefix are consecutive and the last of them is the longest, so one pass sizes and places them.
    uint32_t code = 0, next_sub = 1u << ZI_ROOT;
    int idx = 0;
    int cur_prefix = -1; uint32_t cur_off = 0, cur_bits = 0;
    for (int l = 1; l <= maxl; ++l) {
        for (int c = 0; c < cnt[l]; ++c, ++idx, ++code) {
            const uint32_t sym = sorted[(uint64_t)idx];
            const uint32_t r = zi_rev(code, l);
            if (l <= ZI_ROOT) {
                const uint16_t e = (uint16_t)((l << 9) | sym);
                for (uint32_t i = r + ((uint32_t)lane << l); i < (1u << ZI_ROOT); i += nl << l) tab[i] = e;
                continue;
            }
            const int prefix = (int)(r & ((1u << ZI_ROOT) - 1));
            if (prefix != cur_prefix) {
                // the longest code under this prefix: the last one that shares it (canonical order)
                uint32_t c2 = code; int l2 = l, j = idx, cc = c;
                uint32_t maxbits = (uint32_t)(l - ZI_ROOT);
                while (true) {
                    // advance one code in canonical order
                    ++j; ++cc; ++c2;
                    while (l2 <= maxl && cc >= cnt[l2]) { cc = 0; ++l2; c2 <<= 1; }
                    if (l2 > maxl) break;
                    if ((int)(zi_rev(c2, l2) & ((1u << ZI_ROOT) - 1)) != prefix) break;
                    maxbits = (uint32_t)(l2 - ZI_ROOT);
                }
                if (next_sub + (1u << maxbits) > ZI_TAB) return false;
                cur_prefix = prefix; cur_off = next_sub; cur_bits = maxbits;
                next_sub += 1u << maxbits;
                if (lane == 0) tab[(uint64_t)prefix] = (uint16_t)(0x8000u | (cur_bits << 11) | cur_off);
            }
            const uint32_t sl = (uint32_t)(l - ZI_ROOT);
            const uint16_t e = (uint16_t)((sl << 9) | sym);
            for (uint32_t i = (r >> ZI_ROOT) + ((uint32_t)lane << sl); i < (1u << cur_bits); i += nl << sl) tab[cur_off + i] = e;
        }
        code <<= 1;
    }
    ZI_LANES_SYNC();                                        // the table is whole
    return true;
}

// ---- input: the bit reader over a byte source ------------------------------------------------------------------
// In is a policy with `uint64_t peek8(uint64_t pos)`: the 8 bytes from pos on, little-endian, zero at or past `end`.
// A refill takes as many whole bytes as fit the 64-bit buffer from one such read (the bits above `bn` are those same
// bytes again, so OR-ing the next read over them changes nothing); consumed() > end * 8 means the decoder has used bits
// that are not there.
template <class In> struct zi_bits {
    In& in;
    uint64_t pos;        // next byte to load
    uint64_t end;        // bytes of the view
    uint64_t bb; uint32_t bn;
    ZZ_HD zi_bits(In& i, uint64_t start, uint64_t e) : in(i), pos(start), end(e), bb(0), bn(0) {}
    ZZ_HD void refill()
    {
        if (bn > 56) return;
        bb |= in.peek8(pos) << bn;
        const uint32_t k = (63 - bn) >> 3;
        pos += k; bn += 8 * k;
    }
    ZZ_HD uint64_t consumed() const { return pos * 8 - bn; }
    ZZ_HD bool overrun() const { return pos > end && consumed() > end * 8; }
    ZZ_HD uint32_t get(uint32_t n) { if (bn < n) refill(); const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1)); bb >>= n; bn -= n; return v; }
    ZZ_HD void align() { const uint32_t k = bn & 7; bb >>= k; bn -= k; }
    // restart at byte `p` (behind a stored block)
    ZZ_HD void seek(uint64_t p) { pos = p; bb = 0; bn = 0; }
};

// one symbol from a table; -1 when the bits do not form a code
ZZ_HD inline int zi_decode(const zi_view<uint16_t>& tab, uint64_t& bb, uint32_t& bn)
{
    uint32_t e = tab[bb & ((1u << ZI_ROOT) - 1)];
    if (e & 0x8000u) {
        const uint32_t sb = (e >> 11) & 15u;
        bb >>= ZI_ROOT; bn -= ZI_ROOT;
        e = tab[(e & 0x7FFu) + (uint32_t)(bb & ((1u << sb) - 1))];
    }
    const uint32_t l = (e >> 9) & 15u;
    if (l == 0 || l > bn) return -1;
    bb >>= l; bn -= l;
    return (int)(e & 0x1FFu);
}

// ---- what ends a run of blocks ---------------------------------------------------------------------------------
enum { ZI_RUN_STREAM = 0,     // until the final block (serial path)
       ZI_RUN_INDEXED = 1,    // a packet with a known end: non-final blocks until bit `end * 8`, or the final block
       ZI_RUN_DISCOVER = 2,   // a packet from a candidate start: until `want` bytes at a byte-aligned block end, or the final block
       ZI_RUN_POINT = 3,      // a segment of a point index (zi_pt_segment below): from a bit to a bit, exactly `want` bytes
       ZI_RUN_REACH = 4 };    // measuring a stretch (zi_pt_reach below): from a bit to the first block boundary at or behind `stop`
struct zi_result {
    int err;
    int final;               // the run ended with the final block
    uint64_t end;            // byte (relative to the view) behind the run; the final block's last byte included
    uint64_t out;            // bytes produced
};

// Out is a policy: lit(v), copy(dist, len), stored(in view, pos, len) return ZI_*; `pos` = bytes produced so far.
// `view` is the input [0, n) of the run (the packet or the whole stream) in global memory; `in` the byte source over it.
//
// Pt is a policy known at compile time: what a run does at its block boundaries on top of `mode`. With zi_pt_none (every call
// that names no policy) nothing of it is compiled in.
//   skip             bits of byte `start` that lie in front of the run's first block header: a start that is a bit
//   block(bit, pos)  called in front of every block header: `bit` = consumed() at its BFINAL bit (before any stored-block
//                    alignment), `pos` = bytes produced so far
//   stop, last       ZI_RUN_POINT: the bit where the segment ends; whether it is the stream's last segment
//   end_bit          set by the run: consumed() where it ended
// ZI_RUN_POINT (segment k of a point index, zi_points_check below): blocks from bit start * 8 + skip until the block boundary
// where consumed() == stop; a block that ends behind `stop` is ZI_E_SHAPE; the final block is allowed only in the last segment
// and required there; the segment produces exactly `want` bytes. Behind the last segment R.end is where the trailer starts.
struct zi_pt_none {
    static constexpr bool on = false;
    uint32_t skip; uint64_t stop; bool last; uint64_t end_bit;
    ZZ_HD void block(uint64_t, uint64_t) {}
};
struct zi_pt_segment {
    static constexpr bool on = true;
    uint32_t skip; uint64_t stop; bool last; uint64_t end_bit;
    ZZ_HD void block(uint64_t, uint64_t) {}
};
// ZI_RUN_REACH (a job of the point finder, zi_find_* below): blocks from bit start * 8 + skip until the FIRST block boundary with
// consumed() >= stop, or through the final block; nothing is said about bytes. A run from a false start decodes garbage, so it
// carries `limit`: once consumed() has passed it in mid-block the run ends with ZI_E_GAVEUP (limit = ~0: never). Only a policy
// that says so (zi_pt_reaches) compiles any of this in.
struct zi_pt_reach {
    static constexpr bool on = true;
    uint32_t skip; uint64_t stop; bool last; uint64_t end_bit;
    uint64_t limit;
    ZZ_HD void block(uint64_t, uint64_t) {}
};
template <class Pt> struct zi_pt_reaches { static constexpr bool v = false; };
template <> struct zi_pt_reaches<zi_pt_reach> { static constexpr bool v = true; };
template <class Pt> ZZ_HD inline uint64_t zi_pt_limit(const Pt&) { return ~0ull; }
ZZ_HD inline uint64_t zi_pt_limit(const zi_pt_reach& pt) { return pt.limit; }
template <class In, class Out, class Pt>
ZZ_HD zi_result zi_run(In& in, zi_view<const uint8_t> view, uint64_t start, Out& o, zi_tables& S, int mode, uint64_t want,
                       uint32_t lane, uint32_t nl, Pt& pt)
{
    zi_result R{ ZI_OK, 0, 0, 0 };
    zi_bits<In> b(in, start, view.n);
    if (Pt::on && pt.skip) (void)b.get(pt.skip);
    zi_view<uint16_t> lit{ S.lit, ZI_TAB }, dst{ S.dst, ZI_TAB };
    zi_view<uint8_t> lens{ S.lens, 320 };
    bool any_block = false;
    for (;;) {
        if (any_block) {
            if (mode == ZI_RUN_INDEXED && b.consumed() == view.n * 8) break;
            if (mode == ZI_RUN_DISCOVER && o.pos == want && (b.consumed() & 7) == 0) break;
            if (Pt::on && mode == ZI_RUN_POINT && b.consumed() == pt.stop) break;
            if (zi_pt_reaches<Pt>::v && mode == ZI_RUN_REACH && b.consumed() >= pt.stop) break;
        }
        if (b.consumed() >= view.n * 8) { R.err = ZI_E_DATA; break; }          // the run needs another block that is not there
        if (Pt::on) pt.block(b.consumed(), o.pos);
        b.refill();
        const uint32_t bfinal = b.get(1), type = b.get(2);
        any_block = true;
        if (type == 3) { R.err = ZI_E_DATA; break; }
        if (type == 0) {
            b.align();
            b.refill();
            const uint32_t ln = b.get(16), nln = b.get(16);
            if ((ln ^ nln) != 0xFFFFu || b.overrun()) { R.err = ZI_E_DATA; break; }
            const uint64_t at = b.consumed() >> 3;
            if (at + ln > view.n) { R.err = ZI_E_DATA; break; }
            R.err = o.stored(view, at, ln);
            if (R.err) break;
            b.seek(at + ln);
        } else {
            if (type == 1) {
                if (S.kind != 1) {
                    for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                    zi_build(lit, S, 288, false, false, lane, nl);
                    for (int i = 0; i < 32; ++i) lens[i] = 5;
                    zi_build(dst, S, 32, false, false, lane, nl);
                    S.kind = 1;
                }
            } else {
                S.kind = 0;
                b.refill();
                const uint32_t hlit = b.get(5) + 257, hdist = b.get(5) + 1, hclen = b.get(4) + 4;
                if (hlit > 286 || hdist > 30) { R.err = ZI_E_DATA; break; }
                const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
                for (int i = 0; i < 19; ++i) lens[i] = 0;
                b.refill();
                for (uint32_t i = 0; i < hclen; ++i) { if (b.bn < 3) b.refill(); lens[order[i]] = (uint8_t)b.get(3); }
                if (!zi_build(lit, S, 19, false, false, lane, nl)) { R.err = ZI_E_DATA; break; }   // `lit` holds the code-length code
                // the code lengths go to lens[] (the code-length code is in `lit` already)
                uint32_t idx = 0;
                bool bad = false;
                while (idx < hlit + hdist) {
                    b.refill();
                    const int sym = zi_decode(lit, b.bb, b.bn);
                    if (sym < 0 || sym > 18) { bad = true; break; }
                    if (sym < 16) { lens[idx++] = (uint8_t)sym; continue; }
                    uint32_t rep, val = 0;
                    if (sym == 16) { if (idx == 0) { bad = true; break; } val = lens[idx - 1]; rep = 3 + b.get(2); }
                    else if (sym == 17) rep = 3 + b.get(3);
                    else rep = 11 + b.get(7);
                    if (idx + rep > hlit + hdist) { bad = true; break; }
                    while (rep--) lens[idx++] = (uint8_t)val;
                }
                if (bad || b.overrun()) { R.err = ZI_E_DATA; break; }
                if (lens[256] == 0) { R.err = ZI_E_DATA; break; }                        // no end-of-block code
                if (!zi_build(lit, S, (int)hlit, false, true, lane, nl)) { R.err = ZI_E_DATA; break; }
                for (uint32_t i = 0; i < hdist; ++i) lens[i] = lens[hlit + i];
                if (!zi_build(dst, S, (int)hdist, true, true, lane, nl)) { R.err = ZI_E_DATA; break; }
                S.kind = 2;
            }
            // the symbols of the block; one refill covers a whole length / distance pair (<= 48 bits)
            for (;;) {
                if (zi_pt_reaches<Pt>::v && b.consumed() > zi_pt_limit(pt)) { R.err = ZI_E_GAVEUP; break; }
                if (b.bn < 48) b.refill();
                const int sym = zi_decode(lit, b.bb, b.bn);
                if (sym < 256) {
                    if (sym < 0) { R.err = ZI_E_DATA; break; }
                    R.err = o.lit((uint32_t)sym);
                    if (R.err) break;
                    if (b.overrun()) { R.err = ZI_E_DATA; break; }
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) { R.err = ZI_E_DATA; break; }
                uint32_t len;                                                            // RFC 1951 3.2.5
                if (sym < 265) len = (uint32_t)sym - 254;
                else if (sym == 285) len = 258;
                else { const uint32_t eb = ((uint32_t)sym - 261) >> 2; len = 3 + ((4u | (((uint32_t)sym - 265) & 3)) << eb) + (uint32_t)(b.bb & ((1u << eb) - 1)); b.bb >>= eb; b.bn -= eb; }
                const int ds = zi_decode(dst, b.bb, b.bn);
                if (ds < 0 || ds > 29) { R.err = ZI_E_DATA; break; }
                uint32_t dist;
                if (ds < 4) dist = (uint32_t)ds + 1;
                else { const uint32_t eb = ((uint32_t)ds >> 1) - 1; dist = 1 + ((2u | ((uint32_t)ds & 1)) << eb) + (uint32_t)(b.bb & ((1u << eb) - 1)); b.bb >>= eb; b.bn -= eb; }
                if (b.overrun()) { R.err = ZI_E_DATA; break; }
                R.err = o.copy(dist, len);
                if (R.err) break;
            }
            if (R.err) break;
            if (b.overrun()) { R.err = ZI_E_DATA; break; }
        }
        if (bfinal) { R.final = 1; break; }
        if (mode == ZI_RUN_INDEXED && b.consumed() > view.n * 8) { R.err = ZI_E_DATA; break; }
        if (Pt::on && mode == ZI_RUN_POINT && b.consumed() > pt.stop) { R.err = ZI_E_SHAPE; break; }
        if (zi_pt_reaches<Pt>::v && b.consumed() > zi_pt_limit(pt) && b.consumed() < pt.stop) { R.err = ZI_E_GAVEUP; break; }
    }
    R.end = (b.consumed() + 7) >> 3;
    R.out = o.pos;
    if (Pt::on) pt.end_bit = b.consumed();
    if (R.err) return R;
    if (mode == ZI_RUN_STREAM) { if (!R.final) R.err = ZI_E_DATA; return R; }
    if (zi_pt_reaches<Pt>::v && mode == ZI_RUN_REACH) return R;
    if (Pt::on && mode == ZI_RUN_POINT) {
        if ((R.final != 0) != pt.last || b.consumed() != pt.stop || o.pos != want) R.err = ZI_E_SHAPE;
        return R;
    }
    // a packet: a non-final one is exactly `want` bytes and ends on a byte; the final one holds at most `want`
    if (R.final) { if (o.pos > want) R.err = ZI_E_SHAPE; }
    else if (o.pos != want || (b.consumed() & 7) != 0) R.err = ZI_E_SHAPE;
    return R;
}

template <class In, class Out>
ZZ_HD zi_result zi_run(In& in, zi_view<const uint8_t> view, uint64_t start, Out& o, zi_tables& S, int mode, uint64_t want,
                       uint32_t lane, uint32_t nl)
{
    zi_pt_none pt{ 0, 0, false, 0 };
    return zi_run(in, view, start, o, S, mode, want, lane, nl, pt);
}

// ---- the whole output as the window (serial path; the CPU reference) -----------------------------------------------
// out[0, cap): bytes land at their final place and matches read the bytes in front of them there.
struct zi_fence_none { ZZ_HD void operator()() const {} };
template <class Fence = zi_fence_none> struct zi_out_linear {
    zi_view<uint8_t> out;
    uint64_t pos;
    uint32_t lane, nl;
    Fence fence;
    ZZ_HD int lit(uint32_t v)
    {
        if (pos >= out.n) return ZI_E_SPACE;
        if (lane == 0) out[pos] = (uint8_t)v;
        ++pos;
        return ZI_OK;
    }
    ZZ_HD int copy(uint32_t dist, uint32_t len)
    {
        if (dist > pos) return ZI_E_FAR;
        if (out.n - pos < len) return ZI_E_SPACE;
        fence();                                            // the bytes other lanes wrote are visible
        for (uint32_t i = lane; i < len; i += nl) out[pos + i] = out[pos - dist + (i < dist ? i : i % dist)];
        pos += len;
        return ZI_OK;
    }
    ZZ_HD int stored(const zi_view<const uint8_t>& in, uint64_t at, uint32_t len)
    {
        if (out.n - pos < len) return ZI_E_SPACE;
        for (uint32_t i = lane; i < len; i += nl) out[pos + i] = in[at + i];
        pos += len;
        return ZI_OK;
    }
};

// ---- one packet with its window (phase 1 of the parallel paths) -----------------------------------------------------
// The packet's bytes go to win[0, cap) (LDS on the device). A byte whose match source lies in front of the packet's
// start is PENDING: its bit in `pend` is set and st[pos] holds the absolute position (relative to `base`, plus
// ZI_BIAS) of the byte it copies; a copy from a pending byte copies that pointer. Nothing waits for another packet.
#define ZI_BIAS 32768u
#define ZI_PTR_MASK ((1u << 27) - 1)
struct zi_fence_or {};
template <class Fence, class Or> struct zi_out_packet {
    zi_view<uint8_t> win;          // cap = packet size
    zi_view<uint32_t> pend;        // (cap + 31) / 32 words, zero on entry
    zi_view<uint32_t> st;          // cap pointers (global on the device)
    uint64_t abs;                  // absolute output position of the packet's first byte
    int64_t rel;                   // the same, relative to the batch base the pointers count from
    uint64_t pos;
    uint32_t npend;                // pending bytes this lane wrote
    bool any_pend;                 // uniform: the packet has pending bytes
    uint32_t lane, nl;
    Fence fence; Or bit_or;
    ZZ_HD int lit(uint32_t v)
    {
        if (pos >= win.n) return ZI_E_SHAPE;
        if (lane == 0) win[pos] = (uint8_t)v;
        ++pos;
        return ZI_OK;
    }
    ZZ_HD int copy(uint32_t dist, uint32_t len)
    {
        if (dist > abs + pos) return ZI_E_FAR;                    // in front of the stream
        if (win.n - pos < len) return ZI_E_SHAPE;
        const bool direct = dist > pos;                           // the copy starts in front of the packet
        if (any_pend) fence();                                    // pointers other lanes stored are visible
        if (direct || any_pend) {
            for (uint32_t i = lane; i < len; i += nl) {
                const int64_t s = (int64_t)pos - (int64_t)dist + (int64_t)(i < dist ? i : i % dist);
                const uint64_t q = pos + i;
                if (s < 0) {
                    st[q] = (uint32_t)(rel + s + (int64_t)ZI_BIAS);
                    bit_or(pend, q); ++npend;
                } else if ((pend[(uint64_t)s >> 5] >> (s & 31)) & 1u) {
                    st[q] = st[(uint64_t)s];
                    bit_or(pend, q); ++npend;
                } else {
                    win[q] = win[(uint64_t)s];
                }
            }
            any_pend = true;
        } else {
            for (uint32_t i = lane; i < len; i += nl) win[pos + i] = win[pos - dist + (i < dist ? i : i % dist)];
        }
        pos += len;
        return ZI_OK;
    }
    ZZ_HD int stored(const zi_view<const uint8_t>& in, uint64_t at, uint32_t len)
    {
        if (win.n - pos < len) return ZI_E_SHAPE;
        for (uint32_t i = lane; i < len; i += nl) win[pos + i] = in[at + i];
        pos += len;
        return ZI_OK;
    }
};
struct zi_or_plain {
    ZZ_HD void operator()(zi_view<uint32_t>& m, uint64_t q) const { m[q >> 5] |= 1u << (q & 31); }
};

// ---- a range of an indexed stream (zz_decode_range_device; tests/cxx/inflate_range_harness.cpp runs the same rules) ----
// Bytes [first, first + n) need the packets [k0, k1) that hold them and `h` look-back packets in front: phase 1 runs on
// [kb, k1), kb = k0 - h, with pointers relative to kb * P. A pending byte whose chain leaves the decoded packets at the front is
// EXTERNAL: nothing there is known, so it is not resolved, and a byte that adopts an external pointer is external too (the pointer
// word's round field holds ZI_ROUND_EXTERNAL, which no round number reaches). If an external byte lies inside the requested
// window and kb > 0, the call repeats with a longer look-back; with kb == 0 nothing can be external.
//
// Batches: behind the first batch, a pointer below the batch base reaches at most ZI_BIAS bytes into the batch before it. Those
// bytes are carried in front of the batch's bytes (so `base + y` with y < 0 reads them), and one bit per carried byte says whether
// it is external; for the first batch of an attempt every bit is set.
#define ZI_ROUND_EXTERNAL 31u
// the look-back of the first attempt: one backward extension (levels 2, 3: a match found inside the packet grows backward by at
// most 258 bytes, so its source starts at most 258 bytes in front of the packet). Levels 0 and 1 with cold packets never
// point in front of a packet, so for them these packets are decoded for nothing -- one or two, beside the range's own.
ZZ_HD inline uint64_t zi_range_first_lookback(uint32_t P, uint64_t k0)
{
    const uint64_t h = (258u + (uint64_t)P - 1) / P;
    return h < k0 ? h : k0;
}
// the next look-back after `h` was not enough: four times as many packets, all of them (k0) at the most. A failed attempt costs
// the time one wavefront needs for a packet (milliseconds) while further look-back packets decode beside it on idle CUs, so the
// step is generous; the attempts' work is a geometric series, at most 4/3 of the last one's look-back.
ZZ_HD inline uint64_t zi_range_next_lookback(uint64_t h, uint64_t k0)
{
    if (h >= k0 / 4) return k0;
    return h ? 4 * h : 1;
}
// the target y (relative to the batch base, y < 0: below it, at most ZI_BIAS below) of a pending byte: is it external?
ZZ_HD inline bool zi_range_external(int64_t y, const zi_view<const uint32_t>& carry)
{
    const uint64_t c = (uint64_t)(y + (int64_t)ZI_BIAS);
    return ((carry[c >> 5] >> (c & 31)) & 1u) != 0;
}

// ---- many ranges of one indexed stream in one call (zz_decode_ranges_device; tests/cxx/inflate_ranges_harness.cpp) ---------
// Every read r has its own SEGMENT: packets [k0 - h_r, k1) decoded onto a stage, with pointers relative to the segment's first
// byte. A target below the segment's base is external (there are no batches here, so nothing is carried); a read with an
// external byte inside its window is unfinished and comes back in the next attempt with zi_range_next_lookback's look-back.
// Segments follow one another on the stage in the order of the reads; a WAVE is the run of segments whose first stage packet
// lies in [w * W, (w + 1) * W): whole segments, fewer than W + (longest segment) packets.
enum { ZI_RS_NEW = 0, ZI_RS_AGAIN = 1, ZI_RS_DONE = 2 };        // a read's state: not planned yet, unfinished, settled
// a read's status (= ZZ_OK, ZZ_E_NOSPACE, ZZ_E_ARG, ZZ_E_UNSUPPORTED, ZZ_E_DATA), and "unfinished"
enum { ZI_RV_OK = 0, ZI_RV_NOSPACE = -2, ZI_RV_ARG = -4, ZI_RV_UNSUPPORTED = -5, ZI_RV_DATA = -6, ZI_RV_AGAIN = 1 };
struct zi_read {
    uint64_t h;            // the look-back of the coming (or running) attempt
    uint64_t base;         // first stage packet of its segment in this attempt (an exclusive prefix over the reads)
    uint64_t m;            // bytes it returns (valid once settled ZI_RV_OK)
    uint32_t npk;          // packets of its segment in this attempt; 0: settled, or deferred to a later attempt
    uint32_t state;
    uint32_t fail;         // packets of the segment that failed phase 1 in this attempt
    uint32_t ext;          // external bytes inside its window in this attempt
    uint32_t tries;        // attempts that decoded a segment for it
    int32_t status;
};
// one per stage packet of a wave
struct zi_read_desc {
    uint64_t k;            // the stream's packet
    uint32_t read;
    uint32_t seg0;         // the segment's first stage packet, counted from the wave's
    uint32_t lo, hi;       // bytes [lo, hi) of this packet lie inside the read's window (lo == hi: none)
};
// the packets a read touches: [k0, k1), k1 clipped at the last packet. ZI_RV_ARG for a start behind the index or an overflow.
ZZ_HD inline int zi_ranges_span(uint64_t first, uint64_t nbytes, uint32_t P, uint64_t npk, uint64_t* k0, uint64_t* k1)
{
    if (first / P >= npk || first + nbytes < first) return ZI_RV_ARG;
    *k0 = first / P;
    const uint64_t lastk = nbytes ? (first + nbytes - 1) / P : *k0;
    *k1 = lastk + 1 < npk ? lastk + 1 : npk;
    return ZI_RV_OK;
}
// The plan's share of one read: settles what needs no stage (ZI_RV_ARG, an empty read, a segment above `limit` packets:
// ZI_RV_UNSUPPORTED) and returns the packets of the segment it wants in this attempt (0: none).
ZZ_HD inline uint64_t zi_ranges_plan(zi_read& R, uint64_t first, uint64_t nbytes, uint32_t P, uint64_t npk, uint64_t limit)
{
    if (R.state == ZI_RS_DONE) return 0;
    uint64_t k0 = 0, k1 = 0;
    const int rc = zi_ranges_span(first, nbytes, P, npk, &k0, &k1);
    if (rc) { R.state = ZI_RS_DONE; R.status = rc; return 0; }
    if (nbytes == 0) { R.state = ZI_RS_DONE; R.status = ZI_RV_OK; R.m = 0; return 0; }
    if (R.state == ZI_RS_NEW) { R.h = zi_range_first_lookback(P, k0); R.state = ZI_RS_AGAIN; }
    const uint64_t l = k1 - (k0 - R.h);
    if (l > limit) { R.state = ZI_RS_DONE; R.status = ZI_RV_UNSUPPORTED; return 0; }
    return l;
}
ZZ_HD inline uint64_t zi_ranges_wave(uint64_t base, uint64_t W) { return base / W; }
// bytes [*lo, *hi) of stream packet k lie inside the window [first, first + nbytes) (*lo == *hi: none)
ZZ_HD inline void zi_ranges_cut(uint64_t k, uint64_t first, uint64_t nbytes, uint32_t P, uint32_t* lo, uint32_t* hi)
{
    const uint64_t a = k * P, end = first + nbytes;              // (no overflow: the plan refused it)
    *lo = first > a ? (first - a < P ? (uint32_t)(first - a) : P) : 0u;
    *hi = end > a ? (end - a < P ? (uint32_t)(end - a) : P) : 0u;
    if (*hi < *lo) *hi = *lo;
}
// the descriptor of stage packet j (0-based) of read `r`'s segment, whose first stage packet is `seg0` of the wave. `whole` (a
// checked read): a packet the window touches counts whole, [0, P) -- the widened window of zi_checked_window.
ZZ_HD inline zi_read_desc zi_ranges_desc(const zi_read& R, uint32_t r, uint64_t j, uint32_t seg0, uint64_t first, uint64_t nbytes, uint32_t P,
                                         bool whole = false)
{
    zi_read_desc d;
    d.k = first / P - R.h + j;
    d.read = r; d.seg0 = seg0;
    zi_ranges_cut(d.k, first, nbytes, P, &d.lo, &d.hi);
    if (whole && d.hi > d.lo) { d.lo = 0; d.hi = P; }
    return d;
}
// The verdict on a read after its segment's phase 1 and rounds. `last_out`: bytes the segment's last packet produced (read only
// when the segment reaches the stream's end). ZI_RV_AGAIN: unfinished, R.h grown; otherwise settled with that status.
ZZ_HD inline int zi_ranges_verdict(zi_read& R, uint64_t first, uint64_t nbytes, uint64_t cap, uint32_t P, uint64_t npk, uint64_t limit,
                                   uint32_t last_out)
{
    uint64_t k0 = 0, k1 = 0;
    (void)zi_ranges_span(first, nbytes, P, npk, &k0, &k1);
    ++R.tries;
    int v;
    if (R.fail) v = ZI_RV_DATA;
    else if (R.ext) {
        if (R.h >= k0) v = ZI_RV_DATA;                           // (phase 1 refuses what points in front of the stream)
        else {
            R.h = zi_range_next_lookback(R.h, k0);
            v = k1 - (k0 - R.h) > limit ? ZI_RV_UNSUPPORTED : ZI_RV_AGAIN;
        }
    } else {
        uint64_t have = nbytes;                                  // bytes of the stream from `first` on, if its end is in sight
        if (k1 == npk) { const uint64_t L = (npk - 1) * (uint64_t)P + last_out; have = L > first ? L - first : 0; }
        R.m = nbytes < have ? nbytes : have;
        v = R.m > cap ? ZI_RV_NOSPACE : ZI_RV_OK;
    }
    R.fail = 0; R.ext = 0;
    if (v != ZI_RV_AGAIN) { R.state = ZI_RS_DONE; R.status = v; }
    return v;
}

// ---- the container --------------------------------------------------------------------------------------------
// Header length of a zlib / gzip / raw stream held in h[0, n); <0: -1 not a valid header (or truncated), -2 preset dictionary.
ZZ_HD inline int64_t zi_header(int format, const uint8_t* hp, uint64_t n)
{
    zi_view<const uint8_t> h{ hp, n };
    if (format == 2) return 0;
    if (format == 0) {
        if (n < 2) return -1;
        const uint32_t cmf = h[0], flg = h[1];
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0) return -1;
        if (flg & 0x20) return -2;
        return 2;
    }
    if (format != 1) return -1;
    if (n < 10 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return -1;
    const uint32_t flg = h[3];
    if (flg & 0xE0) return -1;
    uint64_t p = 10;
    if (flg & 4) {                                                 // FEXTRA
        if (p + 2 > n) return -1;
        const uint64_t xlen = h[p] | ((uint64_t)h[p + 1] << 8);
        p += 2 + xlen;
        if (p > n) return -1;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {                       // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (p < n && h[p] != 0) ++p;
        if (p >= n) return -1;
        ++p;
    }
    if (flg & 2) {                                                 // FHCRC: the low 16 bits of the header's CRC-32
        if (p + 2 > n) return -1;
        uint32_t c = ~0u;
        for (uint64_t i = 0; i < p; ++i) {
            c ^= h[i];
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * 0xEDB88320u);
        }
        c = ~c;
        if ((c & 0xFFFFu) != (h[p] | ((uint32_t)h[p + 1] << 8))) return -1;
        p += 2;
    }
    return (int64_t)p;
}

// ---- checksum folds (shared with zz_checksum.h) -----------------------------------------------------------------
#define ZZ_ADLER_MOD 65521u
#define ZZ_CRC_POLY 0xEDB88320u

// ---- GF(2) helpers (host + device) ------------------------------------------------------------------
// a(x)*b(x) mod P(x), bit-reflected representation (bit 31 = x^0)
ZZ_HD inline uint32_t gf2_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ ZZ_CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8*nbytes) mod P
ZZ_HD inline uint32_t gf2_xpow8(uint64_t nbytes)
{
    uint32_t r = 0x80000000u;   // x^0
    uint32_t sq = 0x00800000u;  // x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) r = gf2_mulmod(r, sq);
        sq = gf2_mulmod(sq, sq);
    }
    return r;
}
// crc(A||B) from the finished CRC-32s of A and B and |B|
ZZ_HD inline uint32_t crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2)
{
    return gf2_mulmod(crc1, gf2_xpow8(len2)) ^ crc2;
}
// adler.cpp:5-15: `second` computed with start value 0
ZZ_HD inline uint32_t adler_combine(uint32_t first, uint32_t second, uint64_t len2)
{
    uint64_t a = (uint64_t)(first & 0xFFFF) + (second & 0xFFFF);
    uint64_t b = (uint64_t)(first >> 16) + (second >> 16) + (len2 % ZZ_ADLER_MOD) * (first & 0xFFFF);
    return (uint32_t)(((b % ZZ_ADLER_MOD) << 16) | (a % ZZ_ADLER_MOD));
}

// ---- checked range reads: the packet checksum sidecar (zz_inflate_check.h; tests/cxx/inflate_checked_harness.cpp) ----------
// A sidecar holds one PUBLIC value per packet: zlib's adler32 (start value 1) of the packet's decoded bytes for a zlib stream,
// zlib's crc32 for gzip and raw streams. Inside, a packet's Adler-32 is the start-0 partial (a, b) that folds with adler_combine;
// a CRC-32 partial IS the public value. The sidecar is never trusted: folded in packet order it must give the stream's trailer
// (zi_sidecar_*), and only then is a touched packet's sum on the stage compared with its entry (zi_checked_packet_bad).
enum { ZI_CKS_ADLER = 1, ZI_CKS_CRC = 2 };
ZZ_HD inline int zi_sidecar_kind(int format) { return format == 0 ? ZI_CKS_ADLER : ZI_CKS_CRC; }
// entries of the sidecar of L decoded bytes in packets of P: an empty stream has one (empty) packet
ZZ_HD inline uint64_t zi_sidecar_entries(uint64_t L, uint32_t P)
{
    const uint64_t n = L / P + (L % P ? 1 : 0);
    return n ? n : 1;
}
// decoded bytes of packet k of npk, by the caller's total length (0 when the total does not reach the packet)
ZZ_HD inline uint32_t zi_sidecar_len(uint64_t k, uint64_t L, uint32_t P)
{
    const uint64_t off = k * (uint64_t)P;
    if (off >= L) return 0;
    return L - off < P ? (uint32_t)(L - off) : P;
}
// partial -> public value
ZZ_HD inline uint32_t zi_cks_public(int kind, uint32_t a, uint32_t b, uint32_t len)
{
    if (kind != ZI_CKS_ADLER) return a;
    return (((b + len % ZZ_ADLER_MOD) % ZZ_ADLER_MOD) << 16) | ((a + 1u) % ZZ_ADLER_MOD);
}
// public value -> partial; false: no packet of `len` bytes has this value (a half at or above 65521, or an empty packet with
// anything but the empty value)
ZZ_HD inline bool zi_cks_partial(int kind, uint32_t v, uint32_t len, uint32_t* a, uint32_t* b)
{
    if (kind != ZI_CKS_ADLER) { *a = v; *b = 0; return len != 0 || v == 0; }
    const uint32_t A = v & 0xFFFFu, B = v >> 16;
    *a = (A + ZZ_ADLER_MOD - 1u) % ZZ_ADLER_MOD;
    *b = (B + ZZ_ADLER_MOD - len % ZZ_ADLER_MOD) % ZZ_ADLER_MOD;
    if (A >= ZZ_ADLER_MOD || B >= ZZ_ADLER_MOD) return false;
    return len != 0 || v == 1u;
}
// The window inside which an external byte sends a read back for a longer look-back, as stream positions [*lo, *hi). Unchecked:
// the bytes asked for, as far as the packets [k0, k1) go. Checked: those packets whole -- a packet with an unresolved byte cannot
// be summed, wherever in the packet the byte lies.
ZZ_HD inline void zi_checked_window(bool checked, uint64_t first, uint64_t nbytes, uint32_t P, uint64_t k0, uint64_t k1, uint64_t* lo, uint64_t* hi)
{
    if (checked) { *lo = k0 * P; *hi = k1 * P; return; }
    *lo = first;
    *hi = nbytes < k1 * P - first ? first + nbytes : k1 * P;
}
// The verdict on one touched packet: stream packet k of npk produced `len` bytes (phase 1's word) whose partial is (a, b); `want`
// is its sidecar entry. The stream's last packet must also hold exactly what the caller's total length leaves for it.
ZZ_HD inline bool zi_checked_packet_bad(int kind, uint32_t a, uint32_t b, uint32_t len, uint32_t want, uint64_t k, uint64_t npk, uint64_t L, uint32_t P)
{
    if (k + 1 == npk && (uint64_t)len != L - (npk - 1) * (uint64_t)P) return true;
    return zi_cks_public(kind, a, b, len) != want;
}
// the trailer against the sidecar's fold: `fa`, `fb` the folded start-0 partial of all L bytes (zlib), or the folded CRC-32
ZZ_HD inline bool zi_sidecar_trailer_ok(int format, const uint8_t* t, uint32_t fa, uint32_t fb, uint64_t L)
{
    if (format == 0) {
        const uint32_t want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
        return adler_combine(1u, L ? ((fb << 16) | fa) : 0u, L) == want;
    }
    if (format == 1) {
        const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        return (L ? fa : 0u) == c && l == (uint32_t)L;
    }
    return true;                                                   // a raw stream has no trailer: the sidecar is the caller's own witness
}

// ---- one complete stream: container header, blocks, trailer, checksum (an item of zz_decode_batch_device) -----------
// What zz_decode_device does for one stream between the host and three kernels, done by ONE group of lanes: the header by
// zi_header, the blocks by zi_run onto zi_out_linear over dst[0, cap) (the destination is the window), then exactly
// trailer_len(format) bytes behind the final block and the checksum of the bytes just written, summed by the same lanes
// (they stride the output) and folded over them. Reads only src[0, src_len), writes only dst[0, cap), ends for any input.
//
// L is the lane group's policy:
//   L::in_t, in_t input(p, n)   the byte source over p[0, n) (zi_bits' In)
//   L::fence_t                  zi_out_linear's Fence
//   void sync()                 what every lane wrote to the output is visible to every lane
//   uint64_t sum(uint64_t), uint32_t fold_xor(uint32_t)   over the lanes; every lane gets the result
enum { ZI_ITEM_OK = 0, ZI_ITEM_NOSPACE = -2, ZI_ITEM_UNSUPPORTED = -5, ZI_ITEM_DATA = -6 };   // = ZZ_OK, ZZ_E_NOSPACE, ZZ_E_UNSUPPORTED, ZZ_E_DATA
struct zi_item_result {
    int status;              // ZI_ITEM_*
    uint64_t out;            // decoded bytes (0 unless status is ZI_ITEM_OK)
};

// Adler-32 of out[0, n): lane j sums the bytes j, j + nl, ..; a = sum d_i, b = sum (n - i) d_i on top of the start value 1
template <class L>
ZZ_HD uint32_t zi_adler_lanes(L& w, const zi_view<const uint8_t>& out, uint64_t n, uint32_t lane, uint32_t nl)
{
    uint64_t A = 0, C = 0;                                   // sum d_i and sum (i mod 65521) d_i, both reduced
    uint32_t im = lane % ZZ_ADLER_MOD;                       // i mod 65521 (nl is far below the modulus)
    for (uint64_t i = lane; i < n;) {
        uint64_t a = 0, c = 0;                               // 65536 steps of at most 2^24 each
        for (uint32_t k = 0; k < 65536 && i < n; ++k, i += nl) {
            const uint32_t d = out[i];
            a += d; c += (uint64_t)im * d;
            im += nl; if (im >= ZZ_ADLER_MOD) im -= ZZ_ADLER_MOD;
        }
        A = (A + a) % ZZ_ADLER_MOD; C = (C + c) % ZZ_ADLER_MOD;
    }
    const uint64_t At = w.sum(A) % ZZ_ADLER_MOD, Ct = w.sum(C) % ZZ_ADLER_MOD;
    const uint64_t b = ((n % ZZ_ADLER_MOD) * At + ZZ_ADLER_MOD - Ct) % ZZ_ADLER_MOD;
    return adler_combine(1u, ((uint32_t)b << 16) | (uint32_t)At, n);
}
// CRC-32 of out[0, n): lane j takes the j-th slice (a multiple of four bytes), finishes its CRC and shifts it by the bytes
// behind the slice (crc32_combine with nothing in front); the slices XOR together
template <class L>
ZZ_HD uint32_t zi_crc_lanes(L& w, const zi_view<const uint8_t>& out, uint64_t n, uint32_t lane, uint32_t nl)
{
    const uint64_t slice = ((n + nl - 1) / nl + 3) & ~(uint64_t)3;
    uint64_t b0 = (uint64_t)lane * slice, b1 = b0 + slice;
    if (b0 > n) b0 = n;
    if (b1 > n) b1 = n;
    uint32_t c = 0;
    if (b1 > b0) {
        c = ~0u;
        for (uint64_t i = b0; i < b1; ++i) {
            c ^= out[i];
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * ZZ_CRC_POLY);
        }
        c = gf2_mulmod(~c, gf2_xpow8(n - b1));
    }
    return w.fold_xor(c);
}

template <class L>
ZZ_HD zi_item_result zi_item(L& w, const uint8_t* src, uint64_t src_len, uint8_t* dst, uint64_t cap, int format, zi_tables& S,
                             uint32_t lane, uint32_t nl)
{
    zi_item_result r{ ZI_ITEM_DATA, 0 };
    const int64_t hl = zi_header(format, src, src_len);
    if (hl == -2) { r.status = ZI_ITEM_UNSUPPORTED; return r; }
    if (hl < 0) return r;
    const uint64_t tl = format == 0 ? 4 : format == 1 ? 8 : 0;
    const zi_view<const uint8_t> view{ src + hl, src_len - (uint64_t)hl };     // the blocks and the trailer
    typename L::in_t in = w.input(view.p, view.n);
    zi_out_linear<typename L::fence_t> o{ zi_view<uint8_t>{ dst, cap }, 0, lane, nl, {} };
    S.kind = 0;
    const zi_result R = zi_run(in, view, 0, o, S, ZI_RUN_STREAM, 0, lane, nl);
    if (R.err) { if (R.err == ZI_E_SPACE) r.status = ZI_ITEM_NOSPACE; return r; }
    if (R.end > view.n || view.n - R.end != tl) return r;                      // truncated trailer, or bytes behind it
    const zi_view<const uint8_t> t{ view.p + R.end, tl };
    if (format == 0) {
        w.sync();
        const uint32_t want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
        if (zi_adler_lanes(w, zi_view<const uint8_t>{ dst, R.out }, R.out, lane, nl) != want) return r;
    } else if (format == 1) {
        w.sync();
        const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        if (l != (uint32_t)R.out || zi_crc_lanes(w, zi_view<const uint8_t>{ dst, R.out }, R.out, lane, nl) != c) return r;
    }
    r.status = ZI_ITEM_OK; r.out = R.out;
    return r;
}

// ---- a member file: gzip members back to back (zz_decode_members_device; tests/cxx/inflate_members_harness.cpp) ----------
// src[0, src_len) holds one or more gzip members (RFC 1952 2.2). Every member is judged as zi_item(format = gzip) judges a
// single one; the first byte behind a member's trailer is the next member's 1f or the end of the file -- no padding, and an
// empty file is no member file. The output is the members' bytes one after the other in dst[0, cap); members are judged in
// file order and the first one that fails decides: ZI_ITEM_DATA, or ZI_ITEM_NOSPACE if its bytes pass `cap` before it is
// found invalid. zi_members below IS this definition; the blocked path (zz_inflate_members.h) only reaches it sooner.
struct zi_member_result {
    int status;              // ZI_ITEM_*
    uint64_t out;            // decoded bytes (0 unless status is ZI_ITEM_OK)
    uint64_t used;           // source bytes the member took, trailer included (0 unless status is ZI_ITEM_OK)
};
// zi_item's body for gzip, but bytes may follow the trailer, and the member's length in the source comes back
template <class L>
ZZ_HD zi_member_result zi_member(L& w, const uint8_t* src, uint64_t src_len, uint8_t* dst, uint64_t cap, zi_tables& S,
                                 uint32_t lane, uint32_t nl)
{
    zi_member_result r{ ZI_ITEM_DATA, 0, 0 };
    const int64_t hl = zi_header(1, src, src_len);
    if (hl < 0) return r;
    const zi_view<const uint8_t> view{ src + hl, src_len - (uint64_t)hl };     // the blocks, the trailer and what follows
    typename L::in_t in = w.input(view.p, view.n);
    zi_out_linear<typename L::fence_t> o{ zi_view<uint8_t>{ dst, cap }, 0, lane, nl, {} };
    S.kind = 0;
    const zi_result R = zi_run(in, view, 0, o, S, ZI_RUN_STREAM, 0, lane, nl);
    if (R.err) { if (R.err == ZI_E_SPACE) r.status = ZI_ITEM_NOSPACE; return r; }
    if (R.end > view.n || view.n - R.end < 8) return r;                        // truncated trailer
    const zi_view<const uint8_t> t{ view.p + R.end, 8 };
    w.sync();
    const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (l != (uint32_t)R.out || zi_crc_lanes(w, zi_view<const uint8_t>{ dst, R.out }, R.out, lane, nl) != c) return r;
    r.status = ZI_ITEM_OK; r.out = R.out; r.used = (uint64_t)hl + R.end + 8;
    return r;
}

struct zi_members_result {
    int status;              // ZI_ITEM_*
    uint64_t out;            // decoded bytes of all members (0 unless status is ZI_ITEM_OK)
    uint64_t members;        // members decoded (all of them when status is ZI_ITEM_OK)
};
// the loop over zi_member by one lane group, onto consecutive parts of dst, until the source is used up
template <class L>
ZZ_HD zi_members_result zi_members(L& w, const uint8_t* src, uint64_t src_len, uint8_t* dst, uint64_t cap, zi_tables& S,
                                   uint32_t lane, uint32_t nl)
{
    zi_members_result r{ ZI_ITEM_DATA, 0, 0 };
    while (src_len) {
        const zi_member_result m = zi_member(w, src, src_len, dst, cap, S, lane, nl);
        if (m.status != ZI_ITEM_OK) { r.status = m.status; r.out = 0; return r; }
        src += m.used; src_len -= m.used;                      // (used <= src_len, out <= cap: the member read and wrote inside them)
        dst += m.out; cap -= m.out;
        r.out += m.out; ++r.members;
        w.sync();                                              // every lane has finished with this member's input
    }
    if (r.members == 0) return r;                              // an empty file
    r.status = ZI_ITEM_OK;
    return r;
}

// The member length a header announces (BGZF: the extra subfield `BC`, SLEN 2, holds BSIZE = length - 1), or 0: h[0, n) must
// begin 1f 8b 08 with FEXTRA set and no reserved flag bit, XLEN must lie inside n, and the FIRST subfield B C 2 among the
// subfields inside XLEN counts -- others may stand in front of it (htslib's fixed offset 12 is not assumed). A subfield
// that runs past XLEN, or a length that cannot hold this header, two bytes of blocks and the trailer, gives 0. The length
// is a claim: whoever uses it checks that it stays inside the file, and zi_item judges the member it cuts out.
ZZ_HD inline uint32_t zi_bc_len(const uint8_t* hp, uint64_t n)
{
    if (n < 12) return 0;
    zi_view<const uint8_t> h{ hp, n };
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return 0;
    const uint32_t flg = h[3];
    if (!(flg & 4) || (flg & 0xE0)) return 0;
    const uint64_t xlen = h[10] | ((uint64_t)h[11] << 8);
    const uint64_t end = 12 + xlen;
    if (end > n) return 0;
    for (uint64_t p = 12; p + 4 <= end;) {
        const uint32_t slen = h[p + 2] | ((uint32_t)h[p + 3] << 8);
        if (p + 4 + slen > end) return 0;
        if (h[p] == 0x42 && h[p + 1] == 0x43 && slen == 2) {
            const uint32_t len = (h[p + 4] | ((uint32_t)h[p + 5] << 8)) + 1u;
            return len < end + 2 + 8 ? 0u : len;
        }
        p += 4 + slen;
    }
    return 0;
}

// -- the blocked path's rules (the kernels of zz_inflate_members.h and the harness's host restatement run these) --
// CANDIDATES: every offset i with zi_bc_len(src + i, src_len - i) = len != 0 and i + len <= src_len, ascending.
ZZ_HD inline uint32_t zi_members_candidate(const uint8_t* src, uint64_t src_len, uint64_t i)
{
    const uint32_t len = zi_bc_len(src + i, src_len - i);
    return len && len <= src_len - i ? len : 0u;
}
// CHAIN CHECK, candidate j of m: is its link broken? The file is "blocked and clean" iff no link is: c_0 = 0, c_j + len_j =
// c_(j+1), c_(m-1) + len_(m-1) = src_len. Then the chain of members from offset 0 (the hop below) is the candidate list itself:
// by induction its j-th stop is c_j -- c_0 = 0 is the first stop, and from c_j the header there announces len_j (that is what
// made c_j a candidate), so the next stop is c_j + len_j = c_(j+1), and the last stop's end is src_len.
ZZ_HD inline bool zi_members_link_broken(uint64_t j, uint64_t m, uint64_t c, uint32_t len, uint64_t next, uint64_t src_len)
{
    if (j == 0 && c != 0) return true;
    return c + len != (j + 1 < m ? next : src_len);
}
// HOP: one lane walks the chain from offset 0 with zi_bc_len at each stop and writes the member list (at most `max` members,
// the number of candidates: every stop is one). Returns the members, or 0 when the file is not blocked: a stop at a non-header,
// a length that passes the end, or more stops than candidates.
ZZ_HD inline uint64_t zi_members_hop(const uint8_t* src, uint64_t src_len, uint64_t* offs, uint32_t* lens, uint64_t max)
{
    uint64_t pos = 0, m = 0;
    while (pos < src_len) {
        const uint32_t len = zi_members_candidate(src, src_len, pos);
        if (!len || m >= max) return 0;
        offs[m] = pos; lens[m] = len; ++m;
        pos += len;
    }
    return m;
}
// SLOTS: ISIZE is a member's last four bytes; an exclusive scan of it gives the member's offset `off` in dst, and its slot is
// min(ISIZE, what is left of cap) bytes -- so a lying ISIZE cannot make a member write into its neighbour's slot. m* is the
// first member with off + ISIZE > cap: members behind it are not dealt, and m* itself, short of room, can only answer
// ZI_ITEM_NOSPACE or ZI_ITEM_DATA (ZI_ITEM_OK needs ISIZE bytes decoded).
// (a member of the list lies inside the file with its whole length, and zi_bc_len announces at least 22 bytes)
ZZ_HD inline uint32_t zi_members_isize(const zi_view<const uint8_t>& src, uint64_t c, uint32_t len)
{
    const uint64_t t = c + len - 4;
    return src[t] | ((uint32_t)src[t + 1] << 8) | ((uint32_t)src[t + 2] << 16) | ((uint32_t)src[t + 3] << 24);
}
ZZ_HD inline uint64_t zi_members_slot_cap(uint32_t isize, uint64_t off, uint64_t cap)
{
    const uint64_t left = cap - (cap < off ? cap : off);
    return isize < left ? isize : left;
}
ZZ_HD inline bool zi_members_is_mstar(uint32_t isize, uint64_t off, uint64_t cap) { return off + isize > cap; }
// VERDICT from what k_inflate_items counted over the dealt members: ZI_ITEM_OK (all fine, no m*), ZI_MEMBERS_REJUDGE (one
// member out of room and nothing else wrong -- with an m* that member is m*, see above), or ZI_MEMBERS_SERIAL: the serial path
// decides. ZI_ITEM_OK here implies the serial path's ZI_ITEM_OK with the same bytes: a member that zi_item accepts on exactly
// src[c, c + len) with ISIZE bytes of room is what zi_member reads at c -- the same header, the same bits (a run that ENDS
// inside its view never used a bit behind it), the trailer at the same place -- so the serial loop's stops are the c_j, its
// offsets the scan's, and it ends at src_len.
// A member that is out of room proves less. Its run did not end: zi_run asks for room for a literal before it looks whether
// the literal's bits were there, so zi_item on the cut-out member may have read the zero bits behind the cut where zi_member
// reads the next member's bytes -- and those may spell an end of block, a far distance or no code at all. So "no space" from
// m* is a claim, not the verdict: members 0 .. m* - 1 are proven as above, and zi_members from m* on, over what is left of
// source and room, gives the verdict (ZI_MEMBERS_REJUDGE). For an honest file that is one member's work.
enum { ZI_MEMBERS_SERIAL = 1, ZI_MEMBERS_REJUDGE = 2 };
ZZ_HD inline int zi_members_verdict(bool have_mstar, uint64_t n_data, uint64_t n_nospace)
{
    if (n_data == 0 && n_nospace == 0 && !have_mstar) return ZI_ITEM_OK;
    if (n_data == 0 && n_nospace == 1 && have_mstar) return ZI_MEMBERS_REJUDGE;
    return ZI_MEMBERS_SERIAL;
}

// ---- reads of a member file through an index (zz_decode_members_ranges_device; tests/cxx/inflate_members_ranges_harness.cpp) ----
// The INDEX is `entries` = members + 1 pairs (c_j, u_j): member j is claimed to be src[c_j, c_(j+1)) and to hold the decoded
// bytes [u_j, u_(j+1)) -- its ROOM u_(j+1) - u_j; L = u_(members) is the decoded length. It is an index iff u_0 = 0, c ascends
// strictly, u ascends and c_(members) <= src_len (zi_mr_entry_bad: one entry, one answer); otherwise the call fails as a whole.
// Nothing else of it is trusted: it proposes the cuts, and zi_item judges every member it cuts out -- a member is what the index
// says iff zi_item(gzip) on its bytes, given its room, answers ZI_ITEM_OK with exactly `room` bytes (zi_mr_member_bad).
//
// A READ (first, nbytes, cap) returns m = min(nbytes, L - first) bytes. The plan settles ZI_RV_ARG (first > L, or first + nbytes
// overflows) and ZI_RV_NOSPACE (m > cap); such a read touches nothing, and neither does one with m = 0. Any other read TOUCHES
// the members that hold a byte of [first, first + m): the non-empty members of [j0, j1], j0 = upper_bound(u, first) - 1 (the
// members in front of it that begin at `first` too are empty) and j1 = upper_bound(u, first + m - 1) - 1. Coverage is a
// difference array over the members, +1 at j0 and -1 at j1 + 1, so a read costs two searches whatever it spans.
//
// TOUCHED members, in file order, have ranks t = 0, 1, ..; S_t is the exclusive sum of their rooms and their stage slots follow
// one another: a member with a room above ZZ_MR_STAGE is BIG, takes no room on the stage and is not decoded, and the reads that
// touch it are ZI_RV_UNSUPPORTED. WAVE w holds the ranks with floor(S_t / ZZ_MR_STAGE) = w: less than ZZ_MR_STAGE plus one room
// of stage. The members a read touches have consecutive ranks [a, b), so what a wave holds of a read is ONE interval of its
// stage (zi_mr_cut). F is the exclusive count of members that are not what the index says, G that of big ones, both over the
// ranks: a read is ZI_RV_DATA iff F_b != F_a, else ZI_RV_UNSUPPORTED iff G_b != G_a, else ZI_RV_OK (zi_mr_verdict).
#ifndef ZZ_MR_STAGE
#define ZZ_MR_STAGE (64ull << 20)
#endif
#define ZZ_MR_CHUNK 65536u               // bytes of a read's interval that one workgroup copies at a time
#define ZI_MR_BIG 0x80000000u            // in the touched list: the member is big
struct zi_mr_read {
    uint64_t m;            // bytes the read returns (valid unless status is ZI_RV_ARG)
    uint32_t j0, j1;       // first and last member it touches (valid when `any`)
    int32_t status;        // the plan's: ZI_RV_OK, ZI_RV_ARG, ZI_RV_NOSPACE
    uint32_t any;          // it touches members
};
struct zi_mr_tables {
    zi_view<const uint64_t> idx;       // 2 * entries words
    zi_view<const uint32_t> cnt;       // entries: touched members in front of member j; cnt[members] = their number T
    zi_view<const uint32_t> tlist;     // T: the member of rank t (| ZI_MR_BIG)
    zi_view<const uint64_t> S;         // T + 1
    zi_view<const uint32_t> F, G;      // T + 1 each
};
ZZ_HD inline uint64_t zi_mr_c(const zi_view<const uint64_t>& idx, uint64_t j) { return idx[2 * j]; }
ZZ_HD inline uint64_t zi_mr_u(const zi_view<const uint64_t>& idx, uint64_t j) { return idx[2 * j + 1]; }
ZZ_HD inline uint64_t zi_mr_room(const zi_view<const uint64_t>& idx, uint64_t j) { return zi_mr_u(idx, j + 1) - zi_mr_u(idx, j); }
ZZ_HD inline bool zi_mr_entry_bad(const zi_view<const uint64_t>& idx, uint64_t entries, uint64_t j, uint64_t src_len)
{
    if (j == 0 && zi_mr_u(idx, 0) != 0) return true;
    if (j + 1 == entries) return zi_mr_c(idx, j) > src_len;
    return zi_mr_c(idx, j) >= zi_mr_c(idx, j + 1) || zi_mr_u(idx, j) > zi_mr_u(idx, j + 1);
}
// the first entry whose decoded offset lies behind x (entries: none)
ZZ_HD inline uint64_t zi_mr_upper(const zi_view<const uint64_t>& idx, uint64_t entries, uint64_t x)
{
    uint64_t lo = 0, hi = entries;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (zi_mr_u(idx, mid) <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// PLAN of one read over an index that passed the check (so 1 <= upper_bound(x) <= members for every x < L)
ZZ_HD inline zi_mr_read zi_mr_plan(const zi_view<const uint64_t>& idx, uint64_t entries, uint64_t first, uint64_t nbytes, uint64_t cap)
{
    zi_mr_read R{ 0, 0, 0, ZI_RV_OK, 0 };
    const uint64_t L = zi_mr_u(idx, entries - 1);
    if (first > L || first + nbytes < first) { R.status = ZI_RV_ARG; return R; }
    R.m = nbytes < L - first ? nbytes : L - first;
    if (R.m > cap) { R.status = ZI_RV_NOSPACE; return R; }
    if (R.m == 0) return R;
    const uint64_t members = entries - 1;
    uint64_t a = zi_mr_upper(idx, entries, first), b = zi_mr_upper(idx, entries, first + R.m - 1);
    a = a ? a - 1 : 0; b = b ? b - 1 : 0;
    if (a >= members) a = members - 1;
    if (b >= members) b = members - 1;
    R.j0 = (uint32_t)a; R.j1 = (uint32_t)b; R.any = 1;
    return R;
}
// TOUCHED: what member j is, from its room and the reads that cover it: 0 untouched, 1 touched, 2 touched and big
ZZ_HD inline uint32_t zi_mr_touch(uint64_t room, int32_t cover) { return cover > 0 && room ? (room > ZZ_MR_STAGE ? 2u : 1u) : 0u; }
ZZ_HD inline uint64_t zi_mr_wave(uint64_t S) { return S / ZZ_MR_STAGE; }
// the first rank of [0, T) whose S is at or behind x (T: none): where wave x / ZZ_MR_STAGE begins
ZZ_HD inline uint64_t zi_mr_wave_first(const zi_view<const uint64_t>& S, uint64_t T, uint64_t x)
{
    uint64_t lo = 0, hi = T;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (S[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// DESCRIPTOR of the member of rank t in the wave that begins at rank t0: its bytes in the source and its slot on the stage. A big
// member, and one the index puts outside the source, gets no bytes: zi_item refuses it without reading or writing anything.
struct zi_mr_slot { uint64_t src_off, src_len, stage_off, room; };
ZZ_HD inline zi_mr_slot zi_mr_desc(const zi_mr_tables& T, uint64_t t, uint64_t t0, uint64_t src_len)
{
    const uint32_t e = T.tlist[t];
    const uint64_t j = e & ~ZI_MR_BIG, c0 = zi_mr_c(T.idx, j), c1 = zi_mr_c(T.idx, j + 1);
    if ((e & ZI_MR_BIG) || c1 > src_len || c1 < c0) return zi_mr_slot{ 0, 0, 0, 0 };
    return zi_mr_slot{ c0, c1 - c0, T.S[t] - T.S[t0], zi_mr_room(T.idx, j) };
}
ZZ_HD inline bool zi_mr_member_bad(uint32_t entry, int32_t status, uint64_t out, uint64_t room)
{
    return !(entry & ZI_MR_BIG) && !(status == ZI_ITEM_OK && out == room);
}
// CUT: what the wave of ranks [t0, t1) holds of a read -- `len` bytes at `stage_off` of its stage, for dst + dst_off. Nothing
// for a read the plan settled, one that touches a big member, one whose ranks miss the wave, and one that touches a member of
// this wave that is not what the index says (F is known up to t1 when this is asked). dst_off + len <= m <= cap.
struct zi_mr_piece { uint64_t stage_off, dst_off, len; };
ZZ_HD inline zi_mr_piece zi_mr_cut(const zi_mr_read& R, uint64_t first, const zi_mr_tables& T, uint64_t t0, uint64_t t1)
{
    zi_mr_piece p{ 0, 0, 0 };
    if (R.status != ZI_RV_OK || !R.any) return p;
    const uint64_t a = T.cnt[R.j0], b = T.cnt[(uint64_t)R.j1 + 1];
    if (T.G[b] != T.G[a]) return p;
    const uint64_t ta = a > t0 ? a : t0, tb = b < t1 ? b : t1;
    if (ta >= tb || T.F[tb] != T.F[ta]) return p;
    const uint64_t ja = T.tlist[ta] & ~ZI_MR_BIG, jb = T.tlist[tb - 1] & ~ZI_MR_BIG;
    const uint64_t ua = zi_mr_u(T.idx, ja), ub = zi_mr_u(T.idx, jb);
    const uint64_t d0 = ta == a ? first : ua;                              // decoded offsets of the piece: [d0, d1)
    const uint64_t d1 = tb == b ? first + R.m : zi_mr_u(T.idx, jb + 1);
    const uint64_t s0 = T.S[ta] - T.S[t0] + (d0 - ua), s1 = T.S[tb - 1] - T.S[t0] + (d1 - ub);
    p.stage_off = s0; p.dst_off = d0 - first; p.len = s1 - s0;
    return p;
}
ZZ_HD inline uint64_t zi_mr_chunks(uint64_t len) { return (len + ZZ_MR_CHUNK - 1) / ZZ_MR_CHUNK; }
ZZ_HD inline int zi_mr_verdict(const zi_mr_read& R, const zi_mr_tables& T)
{
    if (R.status != ZI_RV_OK || !R.any) return R.status;
    const uint64_t a = T.cnt[R.j0], b = T.cnt[(uint64_t)R.j1 + 1];
    if (T.F[b] != T.F[a]) return ZI_RV_DATA;
    if (T.G[b] != T.G[a]) return ZI_RV_UNSUPPORTED;
    return ZI_RV_OK;
}

// ---- any stream through a point index (zz_decode_points_device, zz_inflate_points.h; tests/cxx/inflate_points_harness.cpp) ----
// A stream this library did not write has no packets, but its BLOCKS decode independently once one knows where each starts: a
// block start carries no Huffman state, and what crosses it are match sources up to 32 KiB back -- pending bytes, which the rounds
// finish. The POINT INDEX is `entries` = segments + 1 rows (in_bit, out_byte): row k is the header bit of a block (its BFINAL bit,
// counted from the first DEFLATE byte) and the decoded bytes in front of it; row 0 is (0, 0), the last row (the bit behind the
// final block, the decoded length). in_bit ascends strictly, out_byte ascends: a segment may produce no byte (an empty stored
// block), but it never consumes no bit. The index holds no window copies and is never trusted: zi_points_check judges its shape,
// ZI_RUN_POINT every segment, the trailer's checksum the bytes -- and whatever one of them refuses goes to the serial path.
//
// Segments run onto the destination itself (zi_out_segment), BATCHES of whole segments share the pointer array: a batch is a
// greedy run of segments with at most `limit` bytes of output (and at most `max_segs` segments), its base the first segment's
// out_byte; pointers, bitmap bits and the tiles of ZI_POINTS_TILE bytes the rounds work on count from that base. A pointer below
// the base is an earlier batch and therefore final.
#define ZI_POINTS_TILE 32768u
ZZ_HD inline bool zi_points_check(const uint64_t* points, uint64_t entries, uint64_t deflate_len, uint64_t cap, uint64_t limit)
{
    if (entries < 2 || deflate_len > (~0ull >> 3)) return false;
    const zi_view<const uint64_t> p{ points, 2 * entries };
    if (p[0] != 0 || p[1] != 0) return false;
    for (uint64_t k = 0; k + 1 < entries; ++k) {
        if (p[2 * k + 2] <= p[2 * k] || p[2 * k + 3] < p[2 * k + 1]) return false;
        if (p[2 * k + 3] - p[2 * k + 1] > limit) return false;                 // no segment is longer than a batch
    }
    return p[2 * entries - 2] <= deflate_len * 8 && p[2 * entries - 1] <= cap;
}
// the batch that begins with segment k0 ends in front of segment (return value); the index has passed the check
ZZ_HD inline uint64_t zi_points_batches(const uint64_t* points, uint64_t entries, uint64_t k0, uint64_t limit, uint64_t max_segs)
{
    const zi_view<const uint64_t> p{ points, 2 * entries };
    uint64_t k1 = k0 + 1;
    while (k1 + 1 < entries && k1 - k0 < max_segs && p[2 * k1 + 3] - p[2 * k0 + 1] <= limit) ++k1;
    return k1;
}
// pending bytes of a tile: the rounds look at a tile only through its count, and segments and tiles do not line up
ZZ_HD inline uint32_t zi_popc32(uint32_t v)
{
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

// One segment onto the destination: out[0, n) are the segment's bytes -- n is its announced length, so more than that is
// ZI_E_SHAPE and a segment never writes outside its own bytes. zi_out_packet's contract with positions counted from the batch
// base: a byte whose source lies in front of the segment's first byte is PENDING -- its bit in the BATCH's bitmap (at rel + pos)
// and st[rel + pos] = rel + s + ZI_BIAS; a copy from a pending byte copies its pointer, so chains inside a segment are folded
// and every pointer leaves its segment. The window is the destination, as for zi_out_linear: a copy reads what other lanes wrote,
// hence the fence in front of every copy. Or: set(m, q) sets a bit that other lanes and other segments may share a word with,
// test(m, q) reads one that another lane of this segment may have set.
template <class Fence, class Or> struct zi_out_segment {
    zi_view<uint8_t> out;          // the segment's place in the destination
    zi_view<uint32_t> pend;        // the batch's bitmap, zero before phase 1
    zi_view<uint32_t> st;          // the batch's pointers
    uint64_t abs;                  // absolute output position of the segment's first byte
    uint64_t rel;                  // the same, relative to the batch base
    uint64_t pos;
    uint32_t npend;                // pending bytes this lane wrote
    bool any_pend;                 // uniform: the segment has pending bytes
    uint32_t lane, nl;
    Fence fence; Or bits;
    ZZ_HD int lit(uint32_t v)
    {
        if (pos >= out.n) return ZI_E_SHAPE;
        if (lane == 0) out[pos] = (uint8_t)v;
        ++pos;
        return ZI_OK;
    }
    ZZ_HD int copy(uint32_t dist, uint32_t len)
    {
        if (dist > abs + pos) return ZI_E_FAR;                    // in front of the stream
        if (out.n - pos < len) return ZI_E_SHAPE;
        fence();                                                  // bytes, pointers and bits other lanes wrote are visible
        if (dist > pos || any_pend) {                             // the copy starts in front of the segment, or may meet a pending byte
            for (uint32_t i = lane; i < len; i += nl) {
                const int64_t s = (int64_t)pos - (int64_t)dist + (int64_t)(i < dist ? i : i % dist);
                const uint64_t q = pos + i;
                if (s < 0) {
                    st[rel + q] = (uint32_t)((int64_t)rel + s + (int64_t)ZI_BIAS);
                    bits.set(pend, rel + q); ++npend;
                } else if (bits.test(pend, rel + (uint64_t)s)) {
                    st[rel + q] = st[rel + (uint64_t)s];
                    bits.set(pend, rel + q); ++npend;
                } else {
                    out[q] = out[(uint64_t)s];
                }
            }
            any_pend = true;
        } else {
            for (uint32_t i = lane; i < len; i += nl) out[pos + i] = out[pos - dist + (i < dist ? i : i % dist)];
        }
        pos += len;
        return ZI_OK;
    }
    ZZ_HD int stored(const zi_view<const uint8_t>& in, uint64_t at, uint32_t len)
    {
        if (out.n - pos < len) return ZI_E_SHAPE;
        for (uint32_t i = lane; i < len; i += nl) out[pos + i] = in[at + i];
        pos += len;
        return ZI_OK;
    }
};
struct zi_bits_plain {
    ZZ_HD void set(zi_view<uint32_t>& m, uint64_t q) const { m[q >> 5] |= 1u << (q & 31); }
    ZZ_HD bool test(const zi_view<uint32_t>& m, uint64_t q) const { return ((m[q >> 5] >> (q & 31)) & 1u) != 0; }
};

// -- the builder: one sequential pass of one lane, nothing of the output kept (zz_points_index_host) --
// the stream's checksum, summed piece by piece: Adler-32 (zlib), CRC-32 by a byte table (gzip), nothing (raw)
struct zi_sum {
    int format;
    uint32_t a, b, crc;
    uint32_t tab[256];
    ZZ_HD void init(int fmt)
    {
        format = fmt; a = 1; b = 0; crc = ~0u;
        if (fmt != 1) return;
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * ZZ_CRC_POLY);
            tab[i] = c;
        }
    }
    ZZ_HD void add(const zi_view<const uint8_t>& v, uint64_t at, uint64_t n)
    {
        if (format == 0) {
            while (n) {
                const uint64_t m = n < 5552 ? n : 5552;            // zlib's NMAX: the sums stay below 2^32
                for (uint64_t i = 0; i < m; ++i) { a += v[at + i]; b += a; }
                a %= ZZ_ADLER_MOD; b %= ZZ_ADLER_MOD;
                at += m; n -= m;
            }
        } else if (format == 1) {
            const zi_view<const uint32_t> t{ tab, 256 };
            for (uint64_t i = 0; i < n; ++i) crc = (crc >> 8) ^ t[(crc ^ v[at + i]) & 0xFFu];
        }
    }
    // the trailer t[0, 4) or t[0, 8) against the sums over `len` bytes
    ZZ_HD bool trailer_ok(const zi_view<const uint8_t>& t, uint64_t len) const
    {
        if (format == 0) return ((b << 16) | a) == (((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3]);
        if (format != 1) return true;
        const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        return ~crc == c && l == (uint32_t)len;
    }
};
// The out policy of the builder: a ring of ZI_RING bytes is the window (a match reaches 32 KiB back, the ring holds 64), and the
// bytes are summed as the ring turns -- every ZI_RING_TURN bytes, long before they are overwritten -- and then forgotten. One lane.
#define ZI_RING 65536u
#define ZI_RING_TURN 16384u
struct zi_out_ring {
    zi_view<uint8_t> ring;         // ZI_RING bytes
    zi_sum* sum;
    uint64_t pos, summed;
    ZZ_HD void turn()
    {
        const zi_view<const uint8_t> r{ ring.p, ring.n };
        while (summed < pos) {
            const uint64_t at = summed & (ZI_RING - 1);
            uint64_t n = pos - summed;
            if (n > ZI_RING - at) n = ZI_RING - at;
            sum->add(r, at, n);
            summed += n;
        }
    }
    ZZ_HD int lit(uint32_t v)
    {
        ring[pos & (ZI_RING - 1)] = (uint8_t)v;
        ++pos;
        if (pos - summed >= ZI_RING_TURN) turn();
        return ZI_OK;
    }
    ZZ_HD int copy(uint32_t dist, uint32_t len)
    {
        if (dist > pos) return ZI_E_FAR;
        for (uint32_t i = 0; i < len; ++i) ring[(pos + i) & (ZI_RING - 1)] = ring[(pos + i - dist) & (ZI_RING - 1)];
        pos += len;
        if (pos - summed >= ZI_RING_TURN) turn();
        return ZI_OK;
    }
    ZZ_HD int stored(const zi_view<const uint8_t>& in, uint64_t at, uint32_t len)
    {
        while (len) {
            const uint32_t n = len < ZI_RING_TURN ? len : ZI_RING_TURN;
            for (uint32_t i = 0; i < n; ++i) ring[(pos + i) & (ZI_RING - 1)] = in[at + i];
            pos += n; at += n; len -= n;
            turn();
        }
        return ZI_OK;
    }
};
// the input of a host pass: plain memory
struct zi_in_mem {
    zi_view<const uint8_t> v;
    ZZ_HD uint64_t peek8(uint64_t pos) const
    {
        uint64_t r = 0;
        for (uint32_t i = 0; i < 8; ++i) if (pos + i < v.n) r |= (uint64_t)v[pos + i] << (8 * i);
        return r;
    }
};
// The builder's block hook: a point at the first block boundary at or behind every multiple of `spacing` decoded bytes (spacing 1:
// at every block, the empty ones included). Sink: put(in_bit, out_byte), one row.
// the one thinning rule (zi_pt_record, zi_find_rows, zi_points_thin): a boundary at `bit` with `pos` bytes in front of it becomes a
// row iff it is the first at or behind `next`; spacing 1 keeps every boundary, the empty blocks' included
ZZ_HD inline bool zi_points_keep(uint64_t bit, uint64_t pos, uint64_t spacing, uint64_t next) { return !(pos < next && !(spacing == 1 && bit != 0)); }
ZZ_HD inline uint64_t zi_points_next(uint64_t pos, uint64_t spacing) { return pos - pos % spacing + spacing; }
template <class Sink> struct zi_pt_record {
    static constexpr bool on = true;
    uint32_t skip; uint64_t stop; bool last; uint64_t end_bit;
    Sink* sink;
    uint64_t spacing, next;        // the next point: the first boundary with at least `next` bytes in front of it
    ZZ_HD void block(uint64_t bit, uint64_t pos)
    {
        if (!zi_points_keep(bit, pos, spacing, next)) return;
        sink->put(bit, pos);
        next = zi_points_next(pos, spacing);
    }
};
// The whole pass: container header, blocks onto the ring, trailer and checksum -- zi_item's verdict (ZI_ITEM_OK, ZI_ITEM_DATA,
// ZI_ITEM_UNSUPPORTED), the rows through `sink` (the last one included) and the decoded length. ring: ZI_RING bytes.
template <class Sink>
ZZ_HD int zi_points_build(const uint8_t* src, uint64_t src_len, int format, uint64_t spacing, Sink& sink, uint8_t* ring, zi_tables& S,
                          zi_sum& sum, uint64_t* out_len)
{
    const int64_t hl = zi_header(format, src, src_len);
    if (hl == -2) return ZI_ITEM_UNSUPPORTED;
    if (hl < 0 || spacing == 0) return ZI_ITEM_DATA;
    const uint64_t tl = format == 0 ? 4 : format == 1 ? 8 : 0;
    const zi_view<const uint8_t> view{ src + hl, src_len - (uint64_t)hl };     // the blocks and the trailer
    zi_in_mem in{ view };
    sum.init(format);
    zi_out_ring o{ zi_view<uint8_t>{ ring, ZI_RING }, &sum, 0, 0 };
    zi_pt_record<Sink> pt{ 0, 0, false, 0, &sink, spacing, 0 };
    S.kind = 0;
    const zi_result R = zi_run(in, view, 0, o, S, ZI_RUN_STREAM, 0, 0, 1, pt);
    if (R.err) return ZI_ITEM_DATA;
    if (R.end > view.n || view.n - R.end != tl) return ZI_ITEM_DATA;           // truncated trailer, or bytes behind it
    o.turn();
    if (!sum.trailer_ok(zi_view<const uint8_t>{ view.p + R.end, tl }, R.out)) return ZI_ITEM_DATA;
    sink.put(pt.end_bit, R.out);
    *out_len = R.out;
    return ZI_ITEM_OK;
}

// ---- the point index found in parallel (zz_points_index_device, zz_inflate_points_find.h; tests/cxx/points_find_harness.cpp) ----
// Block starts are FOUND in the compressed bytes instead of being reached one after the other. D = the bytes behind the container
// header, trailer included; C = chunk_bytes. cand[0] = 0, and for every chunk c >= 1 (the bits [8cC, min(8(c+1)C, 8|D|))) the
// lowest bit p that passes the TEST: BFINAL = 0, BTYPE = 2 and a dynamic header that zi_run would accept (zi_find_header), no bit
// of it past D. Stored, fixed and final blocks are not searched for. A candidate is only a guess, so the stretches between
// candidates are MEASURED (ZI_RUN_REACH onto zi_out_count: no byte is written) and chained from bit 0: only what is reached from
// bit 0 over block boundaries is the true chain, and only candidates on it become rows.
//
// the first 74 bits at most of a dynamic header, by one lane: lo = the bits p .. p + 63, hi = the bits from p + 64 on (10 used).
// BFINAL / BTYPE, HLIT, HDIST, and the code-length code complete (zi_build(19 symbols, neither empty nor incomplete) accepts
// exactly the length sets whose Kraft sum is one). Rejects nothing zi_find_header accepts.
ZZ_HD inline bool zi_find_prefilter(uint64_t lo, uint64_t hi)
{
    if ((lo & 7u) != 4u) return false;                                // BFINAL 0, BTYPE 2 (binary 10, low bit first)
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = (uint32_t)((lo >> 13) & 15u) + 4;
    uint32_t kraft = 0;                                               // in units of 2^-7
    for (uint32_t i = 0; i < 19; ++i) {
        const uint32_t at = 17 + 3 * i;                               // 17 .. 71: a field may straddle bit 64
        const uint32_t l = (uint32_t)((at < 64 ? (lo >> at) | (at > 61 ? hi << (64 - at) : 0) : hi >> (at - 64)) & 7u);
        if (i < hclen && l) kraft += 128u >> l;
    }
    return kraft == 128u;
}
// the prefilter at bit p over a byte source (In::peek8: zero past the view, so a header cut off by the end reads zeros)
template <class In> ZZ_HD bool zi_find_prefilter_at(In& in, uint64_t p)
{
    const uint64_t b0 = in.peek8(p >> 3), b1 = in.peek8((p >> 3) + 8);
    const uint32_t sh = (uint32_t)(p & 7);
    return zi_find_prefilter(sh ? (b0 >> sh) | (b1 << (64 - sh)) : b0, b1 >> sh);
}
// The dynamic header behind BFINAL / BTYPE exactly as zi_run reads it, the two zi_build calls included: restated, not shared, so
// that zi_run's instantiations stay what they were; the harness holds the two equal at every bit of its small cases.
template <class In>
ZZ_HD bool zi_dyn_header(zi_bits<In>& b, zi_tables& S, uint32_t lane, uint32_t nl)
{
    zi_view<uint16_t> lit{ S.lit, ZI_TAB }, dst{ S.dst, ZI_TAB };
    zi_view<uint8_t> lens{ S.lens, 320 };
    S.kind = 0;
    b.refill();
    const uint32_t hlit = b.get(5) + 257, hdist = b.get(5) + 1, hclen = b.get(4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    for (int i = 0; i < 19; ++i) lens[i] = 0;
    b.refill();
    for (uint32_t i = 0; i < hclen; ++i) { if (b.bn < 3) b.refill(); lens[order[i]] = (uint8_t)b.get(3); }
    if (!zi_build(lit, S, 19, false, false, lane, nl)) return false;
    uint32_t idx = 0;
    while (idx < hlit + hdist) {
        b.refill();
        const int sym = zi_decode(lit, b.bb, b.bn);
        if (sym < 0 || sym > 18) return false;
        if (sym < 16) { lens[idx++] = (uint8_t)sym; continue; }
        uint32_t rep, val = 0;
        if (sym == 16) { if (idx == 0) return false; val = lens[idx - 1]; rep = 3 + b.get(2); }
        else if (sym == 17) rep = 3 + b.get(3);
        else rep = 11 + b.get(7);
        if (idx + rep > hlit + hdist) return false;
        while (rep--) lens[idx++] = (uint8_t)val;
    }
    if (b.overrun()) return false;
    if (lens[256] == 0) return false;
    if (!zi_build(lit, S, (int)hlit, false, true, lane, nl)) return false;
    for (uint32_t i = 0; i < hdist; ++i) lens[i] = lens[hlit + i];
    if (!zi_build(dst, S, (int)hdist, true, true, lane, nl)) return false;
    S.kind = 2;
    return true;
}
// the TEST at bit p of view (p < 8 * view.n), by the whole lane group over its tables
template <class In>
ZZ_HD bool zi_find_header(In& in, zi_view<const uint8_t> view, uint64_t p, zi_tables& S, uint32_t lane, uint32_t nl)
{
    zi_bits<In> b(in, p >> 3, view.n);
    if (p & 7) (void)b.get((uint32_t)(p & 7));
    b.refill();
    if (b.get(1) != 0 || b.get(2) != 2) { S.kind = 0; return false; }
    return zi_dyn_header(b, S, lane, nl);
}
// an Out policy without memory: it counts. A distance cannot be checked here (the decode call does that).
struct zi_out_count {
    uint64_t pos;
    ZZ_HD int lit(uint32_t) { ++pos; return ZI_OK; }
    ZZ_HD int copy(uint32_t, uint32_t len) { pos += len; return ZI_OK; }
    ZZ_HD int stored(const zi_view<const uint8_t>&, uint64_t, uint32_t len) { pos += len; return ZI_OK; }
};
// A JOB measures one stretch; the record is the job on the way in and its result on the way out (32 bytes, in place).
//   in:  a = start bit, b = stop bit (~0: through the final block), c = limit bit (~0: none)
//   out: a = start bit, b = the bit where the run ended, c = the bytes it counted, flags = ZI_FJ_*
enum { ZI_FJ_OK = 1, ZI_FJ_FINAL = 2, ZI_FJ_GAVEUP = 4, ZI_FJ_ERROR = 8,     // a result has exactly one of OK, GAVEUP, ERROR
       ZI_FJ_SENT = 16 };                                                        // (the walk's own: asked for, not there yet)
struct zi_find_job { uint64_t a, b, c; uint32_t flags, pad; };
#define ZI_FIND_NONE (~0ull)
// one job by one lane group: the record is read and then written by the caller
template <class In>
ZZ_HD zi_find_job zi_find_reach(In& in, zi_view<const uint8_t> view, const zi_find_job& j, zi_tables& S, uint32_t lane, uint32_t nl)
{
    zi_out_count o{ 0 };
    zi_pt_reach pt{ (uint32_t)(j.a & 7), j.b, false, 0, j.c };
    S.kind = 0;
    const zi_result R = zi_run(in, view, j.a >> 3, o, S, ZI_RUN_REACH, 0, lane, nl, pt);
    return zi_find_job{ j.a, pt.end_bit, R.out,
                        R.err == ZI_OK ? (uint32_t)ZI_FJ_OK | (R.final ? (uint32_t)ZI_FJ_FINAL : 0u) : R.err == ZI_E_GAVEUP ? (uint32_t)ZI_FJ_GAVEUP : (uint32_t)ZI_FJ_ERROR, 0 };
}
// chunks of |D| = n bytes (an empty D has one), and the limit of a speculative job that is to stop at `stop`: `slack` bytes more
ZZ_HD inline uint64_t zi_find_chunks(uint64_t n, uint64_t C) { const uint64_t k = n / C + (n % C ? 1 : 0); return k ? k : 1; }
ZZ_HD inline uint64_t zi_find_limit(uint64_t stop, uint64_t slack) { return stop == ZI_FIND_NONE || stop + 8 * slack < stop ? ZI_FIND_NONE : stop + 8 * slack; }
// The chain (zi_find_link) and the rows (zi_find_rows). The WALK owns, for ncand candidates (cand[0] = 0, ascending):
//   rc[k]  the result of the job from cand[k] to cand[k + 1] (the last one: through the final block)
//   rr[m]  the result of a REPAIR job that is to stop at cand[m] (m = ncand: through the final block) -- a.start says from where
//   acc    the accepted jobs in chain order: 2 words each, (start bit | candidate flag in bit 63, bytes)
// Link k -> k + 1 holds iff rc[k] ended at cand[k + 1]. Where a job of the true chain ends at a bit e that is no candidate, the
// candidates in front of e are dropped and [e, first candidate at or behind e) is a gap: a repair job from e -- on the true chain by
// construction, so without a limit -- measures it in the next round. A true-chain job that gave up is run again without a limit.
// Behind the first gap the walk goes on PROVISIONALLY, as if the gap's repair landed on its candidate, and asks for the repairs it
// meets there too (with a limit: they may start anywhere), so that the next round finds them done; it accepts nothing there.
// zi_find_link returns what the round decided; jobs it wants are appended to `want` (room for ncand + 2).
enum { ZI_FW_MORE = 0,        // jobs are wanted: run them (one launch), store the results with zi_find_store, link again
       ZI_FW_DONE = 1,        // the chain reached the end of the final block
       ZI_FW_DATA = 2 };      // a job of the true chain ended in an error: the stream's verdict
struct zi_find_walk {
    zi_view<const uint64_t> cand; uint64_t ncand;
    zi_view<zi_find_job> rc, rr;           // ncand, ncand + 1
    zi_view<uint64_t> acc; uint64_t nacc;  // 2 * (2 * ncand + 2) words
    uint64_t pos, m;                       // the confirmed chain's end bit; the first candidate at or behind it
    uint64_t bytes, kept;                  // decoded bytes in front of pos; accepted jobs that started at a candidate
    uint64_t end_bit;                      // ZI_FW_DONE: the bit behind the final block
    uint64_t slack;
};
// the jobs of the first round: one per candidate, job 0 without a limit (it is the true chain). The last candidate's job runs
// through the final block: it gets a limit only where more than ZI_FIND_TAIL bytes of D (n of them) lie behind it.
#define ZI_FIND_TAIL (1ull << 20)
ZZ_HD inline zi_find_job zi_find_first_job(const zi_view<const uint64_t>& cand, uint64_t ncand, uint64_t k, uint64_t slack, uint64_t n)
{
    const uint64_t stop = k + 1 < ncand ? cand[k + 1] : ZI_FIND_NONE;
    uint64_t limit = zi_find_limit(stop, slack);
    if (stop == ZI_FIND_NONE && n * 8 - cand[k] > 8 * ZI_FIND_TAIL) limit = cand[k] + 8 * ZI_FIND_TAIL;
    return zi_find_job{ cand[k], stop, k ? limit : ZI_FIND_NONE, 0, 0 };
}
// a result back into the walk's tables: a job that started at a candidate is rc's, any other rr's (by its start it finds its slot)
ZZ_HD inline void zi_find_store(zi_find_walk& W, const zi_find_job& r)
{
    uint64_t lo = 0, hi = W.ncand;                                   // first candidate at or behind r.a
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (W.cand[mid] < r.a) lo = mid + 1; else hi = mid; }
    if (lo < W.ncand && W.cand[lo] == r.a) W.rc[lo] = r; else W.rr[lo] = r;
}
ZZ_HD inline int zi_find_link(zi_find_walk& W, zi_view<zi_find_job> want, uint64_t* nwant)
{
    *nwant = 0;
    uint64_t q = ZI_FIND_NONE;                                       // the provisional walk starts at candidate q
    for (;;) {                                                        // the confirmed chain
        while (W.m < W.ncand && W.cand[W.m] < W.pos) ++W.m;
        const bool at_cand = W.m < W.ncand && W.cand[W.m] == W.pos;
        zi_find_job& R = at_cand ? W.rc[W.m] : W.rr[W.m];
        const uint64_t stop = at_cand ? (W.m + 1 < W.ncand ? W.cand[W.m + 1] : ZI_FIND_NONE) : (W.m < W.ncand ? W.cand[W.m] : ZI_FIND_NONE);
        const bool have = (R.flags & (ZI_FJ_OK | ZI_FJ_GAVEUP | ZI_FJ_ERROR)) && R.a == W.pos;
        if (!have || (R.flags & ZI_FJ_GAVEUP)) {
            want[(*nwant)++] = zi_find_job{ W.pos, stop, ZI_FIND_NONE, 0, 0 };
            R = zi_find_job{ W.pos, 0, 0, ZI_FJ_SENT, 0 };
            q = at_cand ? W.m + 1 : W.m;
            break;
        }
        if (R.flags & ZI_FJ_ERROR) return ZI_FW_DATA;
        W.acc[2 * W.nacc] = W.pos | (at_cand ? 1ull << 63 : 0); W.acc[2 * W.nacc + 1] = R.c; ++W.nacc;
        if (at_cand) ++W.kept;
        W.bytes += R.c;
        if (R.flags & ZI_FJ_FINAL) { W.end_bit = R.b; return ZI_FW_DONE; }
        if (R.b <= W.pos) return ZI_FW_DATA;                         // (a run consumes at least a block header)
        W.pos = R.b;
    }
    for (uint64_t steps = 0; q < W.ncand && steps <= W.ncand; ++steps) {   // the provisional chain from candidate q
        const zi_find_job& R = W.rc[q];
        if (!(R.flags & ZI_FJ_OK) || (R.flags & ZI_FJ_FINAL) || R.a != W.cand[q] || R.b <= R.a) break;
        uint64_t lo = q + 1, hi = W.ncand;
        while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (W.cand[mid] < R.b) lo = mid + 1; else hi = mid; }
        if (lo < W.ncand && W.cand[lo] == R.b) { q = lo; continue; }  // the link holds (or hops over dropped candidates)
        zi_find_job& G = W.rr[lo];
        if (!(G.flags && G.a == R.b)) {
            const uint64_t stop = lo < W.ncand ? W.cand[lo] : ZI_FIND_NONE;
            want[(*nwant)++] = zi_find_job{ R.b, stop, zi_find_limit(stop, W.slack), 0, 0 };
            G = zi_find_job{ R.b, 0, 0, ZI_FJ_SENT, 0 };
        }
        q = lo;
    }
    return ZI_FW_MORE;
}
// The rows behind ZI_FW_DONE: (0, 0), the accepted candidates with the bytes in front of them (the exclusive scan of the accepted
// jobs' bytes), (end_bit, bytes); thinned by the host builder's rule (zi_pt_record) -- an inner row is kept only if it is the first
// at or behind a multiple of `spacing` bytes. Returns the rows; writes them while they fit `max_rows` (rows == nullptr: counts).
ZZ_HD inline uint64_t zi_find_rows(const zi_find_walk& W, uint64_t spacing, uint64_t* rows, uint64_t max_rows)
{
    uint64_t n = 0, pos = 0, next = 0;
    for (uint64_t i = 0; i < W.nacc; ++i) {
        const uint64_t bit = W.acc[2 * i] & ~(1ull << 63);
        if ((W.acc[2 * i] >> 63) && zi_points_keep(bit, pos, spacing, next)) {
            if (rows && n < max_rows) { rows[2 * n] = bit; rows[2 * n + 1] = pos; }
            ++n;
            next = zi_points_next(pos, spacing);
        }
        pos += W.acc[2 * i + 1];
    }
    if (rows && n < max_rows) { rows[2 * n] = W.end_bit; rows[2 * n + 1] = pos; }
    return n + 1;
}
// the trailer's place and, for gzip, ISIZE: what the call can judge without a decoded byte. t = the last min(n, 8) bytes of D.
ZZ_HD inline bool zi_find_trailer_ok(int format, uint64_t n, uint64_t end_bit, uint64_t out_len, const uint8_t* t)
{
    const uint64_t tl = format == 0 ? 4 : format == 1 ? 8 : 0, end = (end_bit + 7) >> 3;
    if (end > n || n - end != tl) return false;
    if (format != 1) return true;
    return (t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24)) == (uint32_t)out_len;
}

// ---- reads of any stream through a point index with windows (zz_decode_points_ranges_device, zz_inflate_points_ranges.h;
// tests/cxx/inflate_points_ranges_harness.cpp) ----------------------------------------------------------------------------------
// A point index has the shape of a member index: pairs (position in the source, decoded offset), both ascending -- so plan, touched,
// waves, cut, copy and verdict are zi_mr_* with the rows as they are, a SEGMENT where those say member. What a segment needs to
// decode alone is the SIDECAR beside the index, for `segments` = entries - 1:
//   windows  `segments` slots of ZI_PR_WINDOW bytes: slot k holds the decoded bytes [max(0, out_byte[k] - 32768), out_byte[k])
//            right-aligned -- the byte at distance d in front of segment k is slot[ZI_PR_WINDOW - d]; what lies in front of them in
//            the slot is unspecified and never read (zi_out_window reads at distance d only behind `d <= out_byte[k] + pos`)
//   sums     `segments` public checksums (zi_sidecar_kind: adler32 from 1 for zlib, crc32 for gzip and raw) of the segments' bytes
// Neither is trusted. The sums, folded in segment order over the lengths the index gives (64 bits: a segment nobody reads may
// exceed 4 GiB), must give the stream's trailer (zi_pr_join, zi_sidecar_trailer_ok), and every entry must be one a segment of its
// length can have (zi_pr_entry_part); a segment a read touches is decoded whole against its window, summed where it lies on the
// stage and held to its entry: it is what index and sidecar say iff ZI_RUN_POINT accepts it with exactly its room, no distance
// reaches in front of the stream, and the sum of the bytes equals the entry. A wrong window is therefore a mismatch, not wrong bytes.
#define ZI_PR_WINDOW 32768u
// a checksum partial with its length: Adler-32 as the start-0 partial (b << 16 | a), CRC-32 as it is; (0, 0) is nothing
struct zi_pr_part { uint32_t v; uint64_t len; };
ZZ_HD inline zi_pr_part zi_pr_join(int kind, const zi_pr_part& x, const zi_pr_part& y)
{
    return zi_pr_part{ kind == ZI_CKS_ADLER ? adler_combine(x.v, y.v, y.len) : crc32_combine(x.v, y.v, y.len), x.len + y.len };
}
// a partial as the public value a sidecar holds
ZZ_HD inline uint32_t zi_pr_public(int kind, const zi_pr_part& p) { return kind == ZI_CKS_ADLER ? adler_combine(1u, p.v, p.len) : p.v; }
// a sidecar entry of a segment of `len` bytes as a partial; false: no segment of that length has this entry (zi_cks_partial)
ZZ_HD inline bool zi_pr_entry_part(int kind, uint32_t entry, uint64_t len, zi_pr_part* p)
{
    uint32_t a = 0, b = 0;
    const bool ok = zi_cks_partial(kind, entry, len ? (uint32_t)(len % ZZ_ADLER_MOD) + ZZ_ADLER_MOD : 0u, &a, &b);   // (the same residue, and 0 only for 0)
    p->v = kind == ZI_CKS_ADLER ? ((b << 16) | a) : a; p->len = len;
    return ok;
}
// the fold against the trailer t (4 or 8 bytes; raw: none, the sums are the caller's own witness); `all`: every segment joined in order
ZZ_HD inline bool zi_pr_trailer_ok(int format, const uint8_t* t, const zi_pr_part& all)
{
    return zi_sidecar_trailer_ok(format, t, format == 0 ? (all.v & 0xFFFFu) : all.v, format == 0 ? (all.v >> 16) : 0u, all.len);
}
// the DEFLATE bytes of a stream of src_len bytes behind a header of hl: where the last row's bit must end. false: truncated
ZZ_HD inline bool zi_pr_deflate_len(int format, uint64_t src_len, int64_t hl, uint64_t* sn)
{
    const uint64_t tl = format == 0 ? 4 : format == 1 ? 8 : 0;
    if (hl < 0 || src_len < (uint64_t)hl + tl) return false;
    *sn = src_len - (uint64_t)hl - tl;
    return true;
}
// what zi_mr_entry_bad does not ask of the rows: row 0 is the first DEFLATE bit, and the last row's bit ends exactly where the trailer begins
ZZ_HD inline bool zi_pr_ends_ok(uint64_t first_bit, uint64_t last_bit, uint64_t sn) { return first_bit == 0 && last_bit / 8 + (last_bit % 8 ? 1 : 0) == sn; }

// One segment onto its slot of the stage, with its window slot in front of it. out[0, n): n is the segment's room, so more than
// that is ZI_E_SHAPE. A copy whose source lies in front of the segment reads the window slot where it is; one that straddles the
// edge takes its first bytes from the window and the rest from the slot. Nothing is pending. The slot's bytes are read as other
// lanes wrote them, hence the fence in front of every copy; the window is nobody's to write. from_win: bytes this lane took
// from the window.
template <class Fence> struct zi_out_window {
    zi_view<uint8_t> out;          // the segment's slot
    zi_view<const uint8_t> win;    // its window slot: ZI_PR_WINDOW bytes
    uint64_t abs;                  // absolute output position of the segment's first byte
    uint64_t pos;
    uint64_t from_win;
    uint32_t lane, nl;
    Fence fence;
    ZZ_HD int lit(uint32_t v)
    {
        if (pos >= out.n) return ZI_E_SHAPE;
        if (lane == 0) out[pos] = (uint8_t)v;
        ++pos;
        return ZI_OK;
    }
    ZZ_HD int copy(uint32_t dist, uint32_t len)
    {
        if (dist > abs + pos) return ZI_E_FAR;                    // in front of the stream, whatever the slot holds there
        if (out.n - pos < len) return ZI_E_SHAPE;
        fence();                                                  // the bytes other lanes wrote are visible
        if (dist > pos) {                                         // the copy starts `front` bytes in front of the segment: front <= min(abs, 32768)
            const uint32_t front = dist - (uint32_t)pos;
            for (uint32_t i = lane; i < len; i += nl) {
                const uint32_t j = i < dist ? i : i % dist;
                if (j < front) { out[pos + i] = win[ZI_PR_WINDOW - front + j]; ++from_win; }
                else out[pos + i] = out[j - front];
            }
        } else {
            for (uint32_t i = lane; i < len; i += nl) out[pos + i] = out[pos - dist + (i < dist ? i : i % dist)];
        }
        pos += len;
        return ZI_OK;
    }
    ZZ_HD int stored(const zi_view<const uint8_t>& in, uint64_t at, uint32_t len)
    {
        if (out.n - pos < len) return ZI_E_SHAPE;
        for (uint32_t i = lane; i < len; i += nl) out[pos + i] = in[at + i];
        pos += len;
        return ZI_OK;
    }
};

// What the decode kernel is told about the touched segment of rank t in the wave that begins at rank t0: its rows, its window
// slot, its slot on the stage and its room. A big segment is not decoded (`skip`).
struct zi_pr_slot { uint64_t seg, b0, o0, b1, stage_off, room; bool last, skip; };
ZZ_HD inline zi_pr_slot zi_pr_desc(const zi_mr_tables& T, uint64_t entries, uint64_t t, uint64_t t0)
{
    const uint32_t e = T.tlist[t];
    const uint64_t j = e & ~ZI_MR_BIG;
    zi_pr_slot s{ j, zi_mr_c(T.idx, j), zi_mr_u(T.idx, j), zi_mr_c(T.idx, j + 1), 0, 0, j + 2 == entries, (e & ZI_MR_BIG) != 0 };
    if (!s.skip) { s.stage_off = T.S[t] - T.S[t0]; s.room = zi_mr_room(T.idx, j); }
    return s;
}
// The verdict on a decoded segment, in k_inflate_items' words so that zi_mr_member_bad judges it: ZI_ITEM_OK with `room` bytes iff
// the run was accepted (err == 0: ZI_RUN_POINT's shape, its room, no far distance) and the bytes' public sum is the entry
ZZ_HD inline int zi_pr_segment_status(int err, uint64_t out, uint64_t room, uint32_t sum, uint32_t entry)
{
    return err == ZI_OK && out == room && sum == entry ? ZI_ITEM_OK : ZI_ITEM_DATA;
}

// -- the sidecar's builder: a second sequential pass of one lane over a stream and an index somebody made (zz_points_windows_host) --
// The block hook holds every row to the stream: a row's bit must be a block boundary reached with exactly its bytes in front of
// it. There the ring holds the 32 KiB in front of the boundary -- the row's window -- and the sum is cut: the ring is summed up to
// the boundary (zi_out_ring::turn) and the running value is the segment's entry.
struct zi_pt_windows {
    static constexpr bool on = true;
    uint32_t skip; uint64_t stop; bool last; uint64_t end_bit;
    zi_out_ring* o;
    zi_view<const uint64_t> rows; uint64_t entries;
    zi_view<uint8_t> windows; zi_view<uint32_t> sums;      // segments * ZI_PR_WINDOW bytes, segments words
    uint64_t k;                    // the next row to meet
    bool bad;
    // the running sum is segment k - 1's: its entry, and a fresh start
    ZZ_HD void cut()
    {
        o->turn();
        zi_sum& s = *o->sum;
        if (k) sums[k - 1] = s.format == 0 ? ((s.b << 16) | s.a) : ~s.crc;
        s.a = 1; s.b = 0; s.crc = ~0u;
    }
    ZZ_HD void block(uint64_t bit, uint64_t pos)
    {
        if (bad || k + 1 >= entries) return;                       // (the last row is held to the stream's end, behind the run)
        if (rows[2 * k] > bit) return;
        if (rows[2 * k] < bit || rows[2 * k + 1] != pos) { bad = true; return; }     // the row's bit was no boundary, or not with its bytes
        cut();
        const uint64_t have = pos < ZI_PR_WINDOW ? pos : ZI_PR_WINDOW;
        for (uint64_t d = 1; d <= have; ++d) windows[k * ZI_PR_WINDOW + ZI_PR_WINDOW - d] = o->ring[(pos - d) & (ZI_RING - 1)];
        ++k;
    }
};
// The whole pass: zi_points_build's verdict on the stream (header, blocks, trailer's place) and on the rows; then the sums it made
// must fold to the trailer. ZI_ITEM_OK, ZI_ITEM_DATA, ZI_ITEM_UNSUPPORTED (a preset dictionary). ring: ZI_RING bytes.
ZZ_HD inline int zi_points_windows_build(const uint8_t* src, uint64_t src_len, int format, const uint64_t* rows, uint64_t entries,
                                         uint8_t* windows, uint32_t* sums, uint8_t* ring, zi_tables& S, zi_sum& sum)
{
    const int64_t hl = zi_header(format, src, src_len);
    if (hl == -2) return ZI_ITEM_UNSUPPORTED;
    if (hl < 0 || entries < 2) return ZI_ITEM_DATA;
    const uint64_t tl = format == 0 ? 4 : format == 1 ? 8 : 0;
    const uint64_t segments = entries - 1;
    const zi_view<const uint8_t> view{ src + hl, src_len - (uint64_t)hl };     // the blocks and the trailer
    zi_in_mem in{ view };
    const int kind = zi_sidecar_kind(format);
    sum.init(kind == ZI_CKS_ADLER ? 0 : 1);                                    // (a raw stream's segments are summed as gzip's)
    zi_out_ring o{ zi_view<uint8_t>{ ring, ZI_RING }, &sum, 0, 0 };
    zi_pt_windows pt{ 0, 0, false, 0, &o, zi_view<const uint64_t>{ rows, 2 * entries }, entries,
                      zi_view<uint8_t>{ windows, segments * ZI_PR_WINDOW }, zi_view<uint32_t>{ sums, segments }, 0, false };
    S.kind = 0;
    const zi_result R = zi_run(in, view, 0, o, S, ZI_RUN_STREAM, 0, 0, 1, pt);
    if (R.err || pt.bad) return ZI_ITEM_DATA;
    if (R.end > view.n || view.n - R.end != tl) return ZI_ITEM_DATA;           // truncated trailer, or bytes behind it
    if (pt.k != segments || pt.rows[2 * segments] != pt.end_bit || pt.rows[2 * segments + 1] != R.out) return ZI_ITEM_DATA;
    pt.cut();                                                                  // the last segment's entry
    zi_pr_part all{ 0, 0 };
    for (uint64_t j = 0; j < segments; ++j) {
        zi_pr_part p;
        if (!zi_pr_entry_part(kind, pt.sums[j], pt.rows[2 * j + 3] - pt.rows[2 * j + 1], &p)) return ZI_ITEM_DATA;
        all = zi_pr_join(kind, all, p);
    }
    if (all.len != R.out || !zi_pr_trailer_ok(format, view.p + R.end, all)) return ZI_ITEM_DATA;
    return ZI_ITEM_OK;
}

// ---- the sidecar built on the device (zz_points_windows_device, zz_inflate_points_windows.h; tests/cxx/points_windows_harness.cpp) ----
// The same sidecar from batches of the point-index decode: a batch of whole sidecar segments is decoded (ZI_RUN_POINT, the rounds)
// onto a STAGE, and slots and sums are CUT out of it. The stage is `buf`, whose first byte is the absolute output position `org`:
// without a destination it is ZI_PR_WINDOW carried bytes and then the batch (org = base - ZI_PR_WINDOW, negative inside the first
// 32 KiB), with one it is the destination (org = 0). The decode kernels get the pointer position 0 would have, so their far-distance
// check (dist > abs + pos) is the stream's own. A row that thins a finer index (zi_points_thin) is a row of it: the batch is decoded
// with the finer rows between its ends (zi_points_superset), cut by the sidecar's.
ZZ_HD inline int64_t zi_pw_org(uint64_t base, bool onto_dst) { return onto_dst ? 0 : (int64_t)base - (int64_t)ZI_PR_WINDOW; }
// slot k: `zeros` zero bytes, then buf[at, at + ZI_PR_WINDOW - zeros) -- the bytes [out_byte - min(out_byte, 32768), out_byte)
struct zi_pw_place { uint64_t zeros, at; };
ZZ_HD inline zi_pw_place zi_pw_slot_place(uint64_t out_byte, int64_t org)
{
    const uint64_t have = out_byte < ZI_PR_WINDOW ? out_byte : ZI_PR_WINDOW;
    return zi_pw_place{ ZI_PR_WINDOW - have, (uint64_t)((int64_t)(out_byte - have) - org) };
}
ZZ_HD inline void zi_pw_slot_copy(const zi_view<const uint8_t>& buf, const zi_view<uint8_t>& slot, const zi_pw_place& d, uint32_t lane, uint32_t nl)
{
    for (uint64_t j = lane; j < ZI_PR_WINDOW; j += nl) slot[j] = j < d.zeros ? (uint8_t)0 : buf[d.at + (j - d.zeros)];
}
// the public sum of the segment [o0, o1) where it lies on the stage; an empty one: 1 (Adler-32) or 0 (CRC-32), which the sums give
template <class L>
ZZ_HD uint32_t zi_pw_segment_sum(L& w, int kind, const zi_view<const uint8_t>& buf, int64_t org, uint64_t o0, uint64_t o1, uint32_t lane, uint32_t nl)
{
    const uint64_t at = (uint64_t)((int64_t)o0 - org), n = o1 - o0;
    if (n) { (void)buf[at]; (void)buf[at + n - 1]; }
    const zi_view<const uint8_t> seg{ buf.p + at, n };
    return kind == ZI_CKS_ADLER ? zi_adler_lanes(w, seg, n, lane, nl) : zi_crc_lanes(w, seg, n, lane, nl);
}
// every row of `points` occurs in `fine` with the same two numbers, the first and the last rows are the same: one merge walk
ZZ_HD inline bool zi_points_superset(const uint64_t* points, uint64_t entries, const uint64_t* fine, uint64_t fine_entries)
{
    if (entries < 2 || fine_entries < entries) return false;
    if (points[0] != fine[0] || points[1] != fine[1]) return false;
    if (points[2 * entries - 2] != fine[2 * fine_entries - 2] || points[2 * entries - 1] != fine[2 * fine_entries - 1]) return false;
    uint64_t f = 0;
    for (uint64_t k = 0; k < entries; ++k) {
        while (f < fine_entries && !(fine[2 * f] == points[2 * k] && fine[2 * f + 1] == points[2 * k + 1])) ++f;
        if (f == fine_entries) return false;
        ++f;
    }
    return true;
}
// an index thinned to `spacing` by the builder's rule: row 0, the inner rows zi_points_keep keeps, the last row. Returns the rows;
// writes them while they fit `max_rows` (out == nullptr: counts)
ZZ_HD inline uint64_t zi_points_thin(const uint64_t* points, uint64_t entries, uint64_t spacing, uint64_t* out, uint64_t max_rows)
{
    uint64_t n = 0, next = 0;
    for (uint64_t i = 0; i + 1 < entries; ++i) {
        const uint64_t bit = points[2 * i], pos = points[2 * i + 1];
        if (i != 0 && !zi_points_keep(bit, pos, spacing, next)) continue;
        if (out && n < max_rows) { out[2 * n] = bit; out[2 * n + 1] = pos; }
        ++n;
        next = zi_points_next(pos, spacing);
    }
    if (out && n < max_rows) { out[2 * n] = points[2 * entries - 2]; out[2 * n + 1] = points[2 * entries - 1]; }
    return n + 1;
}

// ---- the members of any member file found in parallel (zz_members_find_device, zz_decode_members_found_device,
// zz_inflate_members_find.h; tests/cxx/members_find_harness.cpp) ------------------------------------------------------------------
// A member without `BC` says nothing about its length, so its successor is FOUND instead of reached: every place where a gzip
// header stands is a candidate, every candidate is MEASURED as a member (decoded without writing a byte), and the chain from
// offset 0 over the measured lengths picks the members. The result is defined by the file alone:
//   CANDIDATES  offset 0, and every offset i >= 20 (no member is shorter: ten bytes of header, two of blocks, eight of trailer)
//               with hl = zi_header(gzip, src + i, src_len - i) >= 0 and i + hl + 10 <= src_len; ascending. That is what zi_member
//               accepts as a header, so the start of every member of a valid file is a candidate: the chain below never needs a
//               start that was not found (no gaps and no repair jobs, unlike the point finder above).
//   MEASURE     candidate c: the header, then the blocks through the final one by ZI_RUN_REACH onto zi_out_count (stop ~0), then
//               eight bytes of trailer inside the file whose ISIZE equals the count's low 32 bits. OK gives `used` (header, blocks
//               and trailer) and `out` (the count, 64 bits). CRC-32 and distances cannot be judged: no byte exists yet.
//   WALK        from stop 0: an OK measure at a stop moves it by `used`; stop == src_len ends the walk CLEAN; a stop that is no
//               candidate, a measure that is not OK, or src_len == 0 makes it BROKEN. Candidates the walk steps over are dropped.
// A measure from a false start decodes garbage, so in round 1 every job but job 0 (offset 0 is on the chain) carries a limit: it
// gives up once it has consumed `limit` bytes from its start. A limited job answers what the unlimited one would, or GAVEUP; the
// walk stops at a job that gave up, round 2 runs every job that gave up at or behind that stop again without a limit, and the walk
// then meets no GAVEUP any more: two rounds at most, and what the walk reads -- OK or not, `used`, `out` -- never depends on the
// limit, the rounds or the order the jobs ran in.
ZZ_HD inline bool zi_mf_candidate(const uint8_t* src, uint64_t src_len, uint64_t i)
{
    if (i == 0) return src_len != 0;
    if (i < 20 || i >= src_len) return false;
    const int64_t hl = zi_header(1, src + i, src_len - i);
    return hl >= 0 && i + (uint64_t)hl + 10 <= src_len;
}
// A job's record (zi_find_job, in place): in a = the candidate, c = the limit in bytes from it (ZI_FIND_NONE: none);
// out a = the candidate, b = used, c = out, flags = exactly one of ZI_FJ_OK, ZI_FJ_GAVEUP, ZI_FJ_ERROR.
ZZ_HD inline uint64_t zi_mf_limit(uint64_t k, uint64_t limit_bytes) { return k ? limit_bytes : ZI_FIND_NONE; }
template <class L>
ZZ_HD zi_find_job zi_mf_measure(L& w, const uint8_t* src, uint64_t src_len, const zi_find_job& j, zi_tables& S, uint32_t lane, uint32_t nl)
{
    zi_find_job r{ j.a, 0, 0, ZI_FJ_ERROR, 0 };
    if (j.a >= src_len) return r;
    const int64_t hl = zi_header(1, src + j.a, src_len - j.a);
    if (hl < 0) return r;
    const zi_view<const uint8_t> view{ src + j.a + hl, src_len - j.a - (uint64_t)hl };   // the blocks, the trailer and what follows
    typename L::in_t in = w.input(view.p, view.n);
    zi_out_count o{ 0 };
    const uint64_t limit = j.c == ZI_FIND_NONE || j.c > (~0ull >> 3) ? ZI_FIND_NONE : 8 * (j.c > (uint64_t)hl ? j.c - (uint64_t)hl : 0);
    zi_pt_reach pt{ 0, ZI_FIND_NONE, false, 0, limit };
    S.kind = 0;
    const zi_result R = zi_run(in, view, 0, o, S, ZI_RUN_REACH, 0, lane, nl, pt);
    if (R.err == ZI_E_GAVEUP) { r.flags = ZI_FJ_GAVEUP; return r; }
    if (R.err || !R.final) return r;
    if (R.end > view.n || view.n - R.end < 8) return r;                       // truncated trailer
    const zi_view<const uint8_t> t{ view.p + R.end, 8 };
    const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (l != (uint32_t)R.out) return r;
    r.b = (uint64_t)hl + R.end + 8; r.c = R.out; r.flags = ZI_FJ_OK;
    return r;
}
// The walk over the candidates' records rec[0, nc) (rec[k].a ascending). keep[0, nc) is zero on entry; the walk sets keep[k] for
// the members. It can be called again with the same W after a round: it goes on from its stop.
enum { ZI_MF_MORE = 0,        // the job at the stop gave up: run zi_mf_again's jobs without a limit, then link again
       ZI_MF_CLEAN = 1,       // the chain reached src_len: `members` members, the other candidates dropped
       ZI_MF_BROKEN = 2 };
struct zi_mf_walk {
    uint64_t pos, k;          // the stop; the first candidate that is not in front of it
    uint64_t members, dropped;
};
ZZ_HD inline int zi_mf_link(zi_mf_walk& W, const zi_view<const zi_find_job>& rec, uint64_t nc, uint64_t src_len, zi_view<uint8_t> keep)
{
    if (src_len == 0) return ZI_MF_BROKEN;
    for (;;) {
        while (W.k < nc && rec[W.k].a < W.pos) { ++W.k; ++W.dropped; }
        if (W.k >= nc || rec[W.k].a != W.pos) return ZI_MF_BROKEN;
        const zi_find_job& R = rec[W.k];
        if (R.flags & ZI_FJ_GAVEUP) return ZI_MF_MORE;
        if (!(R.flags & ZI_FJ_OK) || R.b == 0 || R.b > src_len - W.pos) return ZI_MF_BROKEN;
        keep[W.k] = 1; ++W.members; ++W.k;
        W.pos += R.b;
        if (W.pos == src_len) { W.dropped += nc - W.k; return ZI_MF_CLEAN; }
    }
}
// the jobs of round 2: every candidate at or behind the stop whose job gave up. Returns their number; which == nullptr: counts.
ZZ_HD inline uint64_t zi_mf_again(const zi_mf_walk& W, const zi_view<const zi_find_job>& rec, uint64_t nc, uint32_t* which)
{
    uint64_t n = 0;
    for (uint64_t k = W.k; k < nc; ++k) if (rec[k].flags & ZI_FJ_GAVEUP) { if (which) which[n] = (uint32_t)k; ++n; }
    return n;
}
// SLOTS of a clean walk: member j (the j-th kept candidate) begins `off` = the sum of `out` in front of it into the destination and
// gets exactly `out` bytes of room: its count is measured, not claimed. m* is the first member with off + out > cap; the members in
// front of it are dealt to zi_item, and zi_members from m* on gives the verdict. off + out never shrinks, so m* is the one member
// that begins inside cap and ends behind it.
ZZ_HD inline bool zi_mf_dealt(uint64_t out, uint64_t off, uint64_t cap) { return off <= cap && out <= cap - off; }
ZZ_HD inline bool zi_mf_is_mstar(uint64_t out, uint64_t off, uint64_t cap) { return off <= cap && out > cap - off; }

// ---- points inside members: one index over members and blocks (zz_members_points_device,
// zz_inflate_members_points.h; tests/cxx/members_points_harness.cpp) ---------------------------------------------------------------
// The two finders above joined. F = the file, C = chunk_bytes, bits count from F's first byte. The result is defined by F, C and
// `spacing` alone:
//   HEADER CANDIDATES H  zi_mf_candidate's set: offset 0, and every i >= 20 where zi_header(gzip) accepts with ten bytes left behind it
//   BLOCK CANDIDATES B   for every chunk c >= 1 of F the lowest bit that passes zi_find_header, no bit of the header behind F
//                        (the point finder with D = F); chunk 0 has none: bit 0 of F is a gzip header, not a block
//   JOBS                 one per candidate. A header job at i parses the header and measures from bit 8(i + hl); a block job
//                        measures from its bit: ZI_RUN_REACH onto zi_out_count to the first block boundary at or behind its STOP --
//                        the lowest block candidate above the job's first block bit -- or through a final block. A job that ends
//                        with a final block reads the member's ISIZE from the eight bytes behind the block's last byte (an error
//                        if they do not fit in F). A limited job gives up `C` bytes behind its stop, or ZI_FIND_TAIL behind its
//                        first bit where it has no stop; the job at offset 0 and every job the confirmed walk asks for again have
//                        no limit, so no result depends on limits, rounds or scheduling.
//   WALK                 header state at offset i: i must be in H and its job OK; it opens member j with the START row
//                        (8(i + hl) | ZZ_MP_START, off_j). Block state at bit b: if b is in B its job continues the member and
//                        (b, bytes in front of b) is an inner row; otherwise the stretch to the next block candidate is a gap that a
//                        repair job measures (zi_find_link's scheme: behind the first gap the walk goes on provisionally, across
//                        member ends too, and asks for the repairs it meets in the same launch). A job that ends FINAL closes the
//                        member: ISIZE must equal the low 32 bits of the member's count, the END row is (end_bit | ZZ_MP_END,
//                        off_{j+1}), and the next offset is ((end_bit + 7) >> 3) + 8 -- src_len: done, otherwise a header state.
//                        Candidates the walk steps over are dropped; a block candidate that IS an accepted member's first block bit
//                        is absorbed by the START row (neither a row nor dropped).
//   ROWS                 START, inner rows, END per member; `spacing` > 1 thins inner rows only (zi_points_keep on file-absolute
//                        decoded positions, `next` starting again at every START row).
#define ZZ_MP_START (1ull << 63)
#define ZZ_MP_END (1ull << 62)
#define ZZ_MP_BIT(v) ((v) & ~(ZZ_MP_START | ZZ_MP_END))
// A job's record (40 bytes, in place). in: a = the header's offset (ZI_MPJ_HEADER) or the start bit, flags = ZI_MPJ_*;
// out: a as it was, first = the first block bit (8(a + hl), or a), b = the bit where the run ended, c = the bytes it counted,
// isize (FINAL only), flags = the job's kind | exactly one of ZI_FJ_OK, ZI_FJ_GAVEUP, ZI_FJ_ERROR | ZI_FJ_FINAL.
enum { ZI_MPJ_HEADER = 32, ZI_MPJ_NOLIMIT = 64 };
struct zi_mp_job { uint64_t a, b, c, first; uint32_t flags, isize; };
// the lowest block candidate above `bit` (ZI_FIND_NONE: none), and its number
ZZ_HD inline uint64_t zi_mp_above(const zi_view<const uint64_t>& bc, uint64_t nb, uint64_t bit)
{
    uint64_t lo = 0, hi = nb;
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (bc[mid] <= bit) lo = mid + 1; else hi = mid; }
    return lo;
}
ZZ_HD inline uint64_t zi_mp_lower(const zi_view<const uint64_t>& v, uint64_t n, uint64_t x)      // the first element at or behind x
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (v[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// a limited job's limit bit. own_limit (0: none) is the tests': that many bytes behind the job's first bit instead, so that with a
// small one the jobs of the true walk give up too and are run again
ZZ_HD inline uint64_t zi_mp_limit(uint64_t first, uint64_t stop, uint64_t C, uint64_t own_limit)
{
    if (own_limit) return first + 8 * own_limit;
    return stop != ZI_FIND_NONE ? zi_find_limit(stop, C) : first + 8 * ZI_FIND_TAIL;
}
template <class L>
ZZ_HD zi_mp_job zi_mp_measure(L& w, const uint8_t* src, uint64_t n, const zi_view<const uint64_t>& bc, uint64_t nb, uint64_t C,
                              uint64_t own_limit, const zi_mp_job& j, zi_tables& S, uint32_t lane, uint32_t nl)
{
    const uint32_t kind = j.flags & ZI_MPJ_HEADER;
    zi_mp_job r{ j.a, 0, 0, j.a, kind | (uint32_t)ZI_FJ_ERROR, 0 };
    if (kind) {
        if (j.a >= n) return r;
        const int64_t hl = zi_header(1, src + j.a, n - j.a);
        if (hl < 0) return r;
        r.first = 8 * (j.a + (uint64_t)hl);
    }
    if (r.first >= 8 * n) return r;
    const uint64_t s = zi_mp_above(bc, nb, r.first);
    const uint64_t stop = s < nb ? bc[s] : ZI_FIND_NONE;
    const uint64_t limit = (j.flags & ZI_MPJ_NOLIMIT) ? ZI_FIND_NONE : zi_mp_limit(r.first, stop, C, own_limit);
    const zi_view<const uint8_t> view{ src, n };
    typename L::in_t in = w.input(src, n);
    zi_out_count o{ 0 };
    zi_pt_reach pt{ (uint32_t)(r.first & 7), stop, false, 0, limit };
    S.kind = 0;
    const zi_result R = zi_run(in, view, r.first >> 3, o, S, ZI_RUN_REACH, 0, lane, nl, pt);
    r.b = pt.end_bit; r.c = R.out;
    if (R.err == ZI_E_GAVEUP) { r.flags = kind | (uint32_t)ZI_FJ_GAVEUP; return r; }
    if (R.err) return r;
    if (!R.final) { r.flags = kind | (uint32_t)ZI_FJ_OK; return r; }
    if (R.end > n || n - R.end < 8) return r;                                 // truncated trailer
    r.isize = view[R.end + 4] | ((uint32_t)view[R.end + 5] << 8) | ((uint32_t)view[R.end + 6] << 16) | ((uint32_t)view[R.end + 7] << 24);
    r.flags = kind | (uint32_t)ZI_FJ_OK | (uint32_t)ZI_FJ_FINAL;
    return r;
}
// The WALK owns, for nh header candidates hc (ascending offsets) and nb block candidates bc (ascending bits):
//   rh[k]  the header job of hc[k];  rb[m]  the block job of bc[m];  rr[m]  a repair job whose stop is bc[m] (m = nb: none)
//   acc    the rows in order, not thinned: 2 words each (room for 2 * nh + nb rows)
// zi_mp_link returns ZI_FW_MORE / DONE / DATA as zi_find_link does; jobs it wants are appended to `want` (room for nh + nb + 2).
struct zi_mp_walk {
    zi_view<const uint64_t> hc; uint64_t nh; zi_view<const uint64_t> bc; uint64_t nb;
    zi_view<zi_mp_job> rh, rb, rr;
    zi_view<uint64_t> acc; uint64_t nacc;
    uint64_t src_len;
    int block;                              // the state: 0 a header at offset `pos`, 1 a block at bit `pos`
    uint64_t pos, k, m;                     // k, m: the first header / block candidate that is not in front of the walk
    uint64_t bytes, origin;                 // decoded bytes in front of pos; in front of the open member
    uint64_t members, inner, absorbed;
};
ZZ_HD inline zi_mp_job zi_mp_first_job(const zi_mp_walk& W, uint64_t i)        // round 1: job i of nh + nb
{
    if (i < W.nh) return zi_mp_job{ W.hc[i], 0, 0, 0, (uint32_t)ZI_MPJ_HEADER | (W.hc[i] == 0 ? (uint32_t)ZI_MPJ_NOLIMIT : 0u), 0 };
    return zi_mp_job{ W.bc[i - W.nh], 0, 0, 0, 0, 0 };
}
ZZ_HD inline void zi_mp_store(zi_mp_walk& W, const zi_mp_job& r)
{
    if (r.flags & ZI_MPJ_HEADER) { const uint64_t k = zi_mp_lower(W.hc, W.nh, r.a); if (k < W.nh && W.hc[k] == r.a) W.rh[k] = r; return; }
    const uint64_t m = zi_mp_lower(W.bc, W.nb, r.a);
    if (m < W.nb && W.bc[m] == r.a) W.rb[m] = r; else W.rr[m] = r;
}
ZZ_HD inline bool zi_mp_have(const zi_mp_job& R, uint64_t a) { return (R.flags & (ZI_FJ_OK | ZI_FJ_GAVEUP | ZI_FJ_ERROR)) && R.a == a; }
ZZ_HD inline uint64_t zi_mp_next_offset(uint64_t end_bit) { return ((end_bit + 7) >> 3) + 8; }
ZZ_HD inline int zi_mp_link(zi_mp_walk& W, zi_view<zi_mp_job> want, uint64_t* nwant)
{
    *nwant = 0;
    if (W.src_len == 0) return ZI_FW_DATA;
    bool pblock = false; uint64_t ppos = 0;                          // where the provisional walk starts (pblock: at candidate ppos)
    for (;;) {                                                        // the confirmed walk
        zi_mp_job* R;
        bool at_cand = false;
        if (!W.block) {
            while (W.k < W.nh && W.hc[W.k] < W.pos) ++W.k;
            if (W.k >= W.nh || W.hc[W.k] != W.pos) return ZI_FW_DATA;          // what stands behind a trailer is no header
            R = &W.rh[W.k];
        } else {
            while (W.m < W.nb && W.bc[W.m] < W.pos) ++W.m;
            at_cand = W.m < W.nb && W.bc[W.m] == W.pos;
            R = at_cand ? &W.rb[W.m] : &W.rr[W.m];
        }
        if (!zi_mp_have(*R, W.pos) || (R->flags & ZI_FJ_GAVEUP)) {
            const bool gave = zi_mp_have(*R, W.pos);
            const uint64_t first = gave ? R->first : W.pos;
            want[(*nwant)++] = zi_mp_job{ W.pos, 0, 0, 0, (W.block ? 0u : (uint32_t)ZI_MPJ_HEADER) | (uint32_t)ZI_MPJ_NOLIMIT, 0 };
            *R = zi_mp_job{ W.pos, 0, 0, first, (W.block ? 0u : (uint32_t)ZI_MPJ_HEADER) | (uint32_t)ZI_FJ_SENT, 0 };
            if (!W.block && !gave) return ZI_FW_MORE;                 // (round 1 runs every header job: not reached)
            pblock = true; ppos = zi_mp_above(W.bc, W.nb, first);     // as if the job landed on the candidate above its first bit
            break;
        }
        if (R->flags & ZI_FJ_ERROR) return ZI_FW_DATA;
        if (!W.block) {                                               // the job opens a member
            W.origin = W.bytes;
            W.acc[2 * W.nacc] = R->first | ZZ_MP_START; W.acc[2 * W.nacc + 1] = W.bytes; ++W.nacc;
            ++W.members;
            while (W.m < W.nb && W.bc[W.m] < R->first) ++W.m;
            if (W.m < W.nb && W.bc[W.m] == R->first) { ++W.absorbed; ++W.m; }
            W.block = 1;
        } else if (at_cand) {
            W.acc[2 * W.nacc] = W.pos; W.acc[2 * W.nacc + 1] = W.bytes; ++W.nacc;
            ++W.inner;
        }
        W.bytes += R->c;
        if (R->flags & ZI_FJ_FINAL) {                                 // the job closes the member
            if (R->isize != (uint32_t)(W.bytes - W.origin)) return ZI_FW_DATA;
            W.acc[2 * W.nacc] = R->b | ZZ_MP_END; W.acc[2 * W.nacc + 1] = W.bytes; ++W.nacc;
            const uint64_t next = zi_mp_next_offset(R->b);
            if (next > W.src_len) return ZI_FW_DATA;
            if (next == W.src_len) return ZI_FW_DONE;
            W.block = 0; W.pos = next;
            continue;
        }
        if (R->b <= R->first) return ZI_FW_DATA;                      // (a run consumes at least a block header)
        W.pos = R->b;
    }
    for (uint64_t steps = 0; steps <= W.nh + W.nb; ++steps) {         // the provisional walk: it accepts nothing
        const zi_mp_job* R;
        if (pblock) {
            if (ppos >= W.nb) break;
            R = &W.rb[ppos];
            if (!(R->flags & ZI_FJ_OK) || R->a != W.bc[ppos]) break;
        } else {
            const uint64_t k = zi_mp_lower(W.hc, W.nh, ppos);
            if (k >= W.nh || W.hc[k] != ppos) break;
            R = &W.rh[k];
            if (!(R->flags & ZI_FJ_OK) || R->a != ppos) break;
        }
        if (R->flags & ZI_FJ_FINAL) {
            pblock = false; ppos = zi_mp_next_offset(R->b);
            if (ppos >= W.src_len) break;
            continue;
        }
        if (R->b <= R->first) break;
        const uint64_t lo = zi_mp_lower(W.bc, W.nb, R->b);
        if (!(lo < W.nb && W.bc[lo] == R->b)) {                       // a gap: its repair, limited (it may start anywhere)
            zi_mp_job& G = W.rr[lo];
            if (!(G.flags && G.a == R->b)) {
                want[(*nwant)++] = zi_mp_job{ R->b, 0, 0, 0, 0, 0 };
                G = zi_mp_job{ R->b, 0, 0, R->b, ZI_FJ_SENT, 0 };
            }
        }
        pblock = true; ppos = lo;
    }
    return ZI_FW_MORE;
}
ZZ_HD inline uint64_t zi_mp_dropped(const zi_mp_walk& W) { return W.nh + W.nb - W.members - W.inner - W.absorbed; }
// The rows behind ZI_FW_DONE, thinned. Returns the rows; writes them while they fit `max_rows` (rows == nullptr: counts).
ZZ_HD inline uint64_t zi_mp_rows(const zi_mp_walk& W, uint64_t spacing, uint64_t* rows, uint64_t max_rows)
{
    uint64_t n = 0, next = 0;
    for (uint64_t i = 0; i < W.nacc; ++i) {
        const uint64_t bit = W.acc[2 * i], pos = W.acc[2 * i + 1];
        if (!(bit & (ZZ_MP_START | ZZ_MP_END)) && !zi_points_keep(bit, pos, spacing, next)) continue;
        if (!(bit & ZZ_MP_END)) next = zi_points_next(pos, spacing);
        if (rows && n < max_rows) { rows[2 * n] = bit; rows[2 * n + 1] = pos; }
        ++n;
    }
    return n;
}
// The START / END rows as zz_members_find_device's pairs (file offset, decoded offset): c_0 = 0, c_{j+1} = behind END_j's trailer.
// Returns the pairs (members + 1), or 0 where the rows are no member point index; writes them while they fit.
ZZ_HD inline uint64_t zi_mp_to_index(const uint64_t* points, uint64_t entries, uint64_t* index, uint64_t max_entries)
{
    uint64_t n = 0, c = 0;
    bool open = false;
    for (uint64_t i = 0; i < entries; ++i) {
        const uint64_t bit = points[2 * i], pos = points[2 * i + 1];
        if ((bit & ZZ_MP_START) && (bit & ZZ_MP_END)) return 0;
        if (bit & ZZ_MP_START) {
            if (open) return 0;
            open = true;
            if (index && n < max_entries) { index[2 * n] = c; index[2 * n + 1] = pos; }
            ++n;
        } else if (bit & ZZ_MP_END) {
            if (!open) return 0;
            open = false;
            c = zi_mp_next_offset(ZZ_MP_BIT(bit));
            if (i + 1 == entries) { if (index && n < max_entries) { index[2 * n] = c; index[2 * n + 1] = pos; } ++n; }
        } else if (!open) return 0;
    }
    return open || entries == 0 ? 0 : n;
}

// ---- decode through a member point index (zz_decode_members_points_device, zz_inflate_members_decode.h;
// tests/cxx/members_points_decode_harness.cpp) ------------------------------------------------------------------------------------
// The rows are never trusted: they decide speed, not the result, which is zi_members' for every input.
//   THE ROWS ARE AN INDEX (zi_mpd_plan)  START, inner rows, END per member (zi_mp_to_index's rule); masked bits ascend strictly over
//                        the whole array; every START bit is a multiple of 8; out_byte ascends from 0 and every END's equals the next
//                        START's; with c_0 = 0 and c_{j+1} = zi_mp_next_offset(end_j): c_j + 10 <= start_j / 8, and the last c is
//                        src_len. Anything else: the serial path decides on the whole file.
//   SEGMENTS             a pair of neighbouring rows whose first is no END row: one descriptor (zi_mpd_seg) -- its two bits with the
//                        flags masked off, its bytes [o0, o1), its member's decoded origin off_j, whether it is the member's last.
//   DEALT                member j is dealt if it lies in front of m*, the first member whose bytes pass `cap` or that holds a segment
//                        of more than `limit` bytes (zi_mpd_mstar). Batches are greedy runs of dealt descriptors (zi_mpd_batch).
//   PROVEN               a dealt member is proven iff (1) zi_header(gzip) at c_j ends exactly at start_j / 8, (2) every segment of it
//                        runs ZI_RUN_POINT from its bit to exactly the next row's bit with exactly its room, the final block in its
//                        last segment and nowhere else, NO DISTANCE REACHING IN FRONT OF off_j (zi_out_segment::abs = o0 - off_j: abs
//                        serves the ZI_E_FAR test and nothing else), (3) the CRC-32 of its segments' bytes, joined in order
//                        (zi_pr_join), is the trailer's and (4) ISIZE is the low 32 bits of off_{j+1} - off_j (zi_mpd_verdict).
// With f the first dealt member that is not proven, or m*: no f is ZI_ITEM_OK with the last row's out_byte; otherwise zi_members from
// (c_f, off_f) over what is left of source, destination and room answers. Why that is zi_members' answer: DESIGN.md 23.
struct zi_mpd_seg { uint64_t b0, b1, o0, o1, origin, member_last; };       // member_last = member << 1 | the member's last segment
struct zi_mpd_member {
    uint64_t c, first, end;          // its first byte in the file, its first block's byte, the bit behind its final block
    uint64_t off, out;               // decoded bytes in front of it, its own
    uint64_t seg0, nseg, longest;    // its descriptors, and its longest segment's bytes
};
// The rows as members and descriptors. Returns false where the rows are no index. Counts (*nmem, *nseg) are always set for an index;
// mem / seg are written while they fit (null: counts only). One row per turn: entries turns.
ZZ_HD inline bool zi_mpd_plan(const uint64_t* points, uint64_t entries, uint64_t src_len, zi_mpd_member* mem, uint64_t max_mem,
                              zi_mpd_seg* seg, uint64_t max_seg, uint64_t* nmem, uint64_t* nseg)
{
    *nmem = 0; *nseg = 0;
    if (entries < 2 || src_len > (~0ull >> 3)) return false;
    if (zi_mp_to_index(points, entries, nullptr, 0) == 0) return false;    // START, inner rows, END per member
    const zi_view<const uint64_t> p{ points, 2 * entries };
    uint64_t c = 0, m = 0, s = 0;
    zi_mpd_member cur{ 0, 0, 0, 0, 0, 0, 0, 0 };
    for (uint64_t i = 0; i < entries; ++i) {
        const uint64_t raw = p[2 * i], bit = ZZ_MP_BIT(raw), pos = p[2 * i + 1];
        if (i == 0 ? pos != 0 : (bit <= ZZ_MP_BIT(p[2 * i - 2]) || pos < p[2 * i - 1])) return false;
        if (raw & ZZ_MP_START) {
            if ((bit & 7) != 0 || bit / 8 < c + 10) return false;
            if (i && pos != p[2 * i - 1]) return false;                    // the gap between two members holds no byte
            cur = zi_mpd_member{ c, bit / 8, 0, pos, 0, s, 0, 0 };
            continue;
        }
        // an inner row or an END row closes the segment its predecessor opened
        const uint64_t b0 = ZZ_MP_BIT(p[2 * i - 2]), o0 = p[2 * i - 1];
        const bool last = (raw & ZZ_MP_END) != 0;
        if (seg && s < max_seg) seg[s] = zi_mpd_seg{ b0, bit, o0, pos, cur.off, (m << 1) | (last ? 1u : 0u) };
        ++s; ++cur.nseg;
        if (pos - o0 > cur.longest) cur.longest = pos - o0;
        if (!last) continue;
        cur.end = bit; cur.out = pos - cur.off;
        c = zi_mp_next_offset(bit);
        if (c > src_len) return false;
        if (mem && m < max_mem) mem[m] = cur;
        ++m;
    }
    if (c != src_len) return false;
    *nmem = m; *nseg = s;
    return true;
}
// m*: the first member whose bytes pass cap or that holds a segment longer than a batch (nmem: none). off + out never shrinks.
ZZ_HD inline uint64_t zi_mpd_mstar(const zi_mpd_member* mem, uint64_t nmem, uint64_t cap, uint64_t limit)
{
    for (uint64_t j = 0; j < nmem; ++j) if (mem[j].off + mem[j].out > cap || mem[j].longest > limit) return j;
    return nmem;
}
// the batch that begins with descriptor k0 < n ends in front of descriptor (return value) > k0: zi_points_batches' rule on descriptors
// (no dealt segment is longer than `limit`, and the members' bytes lie back to back, so a batch holds at most `limit` bytes)
ZZ_HD inline uint64_t zi_mpd_batch(const zi_mpd_seg* seg, uint64_t n, uint64_t k0, uint64_t limit, uint64_t max_segs)
{
    uint64_t k1 = k0 + 1;
    while (k1 < n && k1 - k0 < max_segs && seg[k1].o1 - seg[k0].o0 <= limit) ++k1;
    return k1;
}
// One descriptor's phase 1 onto the destination (absolute positions), by one lane group: zi_out_segment with the member's origin.
// `in` reads the file src[0, n); the batch's bitmap and pointers count from `base`. Returns the run's result (err == 0: condition 2).
template <class Fence, class Bits, class In>
ZZ_HD zi_result zi_mpd_segment(In& in, const uint8_t* src, uint64_t n, const zi_mpd_seg& d, uint8_t* dst, uint64_t base, uint32_t* pend,
                               uint64_t words, uint32_t* st, uint64_t nbytes, zi_tables& S, uint32_t lane, uint32_t nl, uint32_t* npend)
{
    const zi_view<const uint8_t> view{ src, n };
    zi_out_segment<Fence, Bits> o{ zi_view<uint8_t>{ dst + d.o0, d.o1 - d.o0 }, zi_view<uint32_t>{ pend, words }, zi_view<uint32_t>{ st, nbytes },
                                   d.o0 - d.origin, d.o0 - base, 0, 0, false, lane, nl, {}, {} };
    zi_pt_segment pt{ (uint32_t)(d.b0 & 7), d.b1, (d.member_last & 1) != 0, 0 };
    S.kind = 0;
    const zi_result R = zi_run(in, view, d.b0 >> 3, o, S, ZI_RUN_POINT, d.o1 - d.o0, lane, nl, pt);
    *npend = o.npend;
    return R;
}
// The verdict's fold. A lane's run: the sums of `per` consecutive segments of the member from its lane * per-th on, joined in
// order; `ok` is cleared by a segment whose run was refused (or never launched). No lane joins more than per = ceil(nseg / nl) sums.
ZZ_HD inline zi_pr_part zi_mpd_fold_run(const zi_mpd_member& M, const zi_mpd_seg* seg, const uint32_t* sums, const uint8_t* segok,
                                        uint32_t lane, uint32_t nl, bool* ok)
{
    const uint64_t per = (M.nseg + nl - 1) / nl;
    uint64_t k0 = M.seg0 + (uint64_t)lane * per, k1 = k0 + per;
    if (k0 > M.seg0 + M.nseg) k0 = M.seg0 + M.nseg;
    if (k1 > M.seg0 + M.nseg) k1 = M.seg0 + M.nseg;
    zi_pr_part acc{ 0, 0 };
    for (uint64_t k = k0; k < k1; ++k) {
        if (!segok[k]) *ok = false;
        acc = zi_pr_join(ZI_CKS_CRC, acc, zi_pr_part{ sums[k], seg[k].o1 - seg[k].o0 });
    }
    return acc;
}
// one step of the tree over the lanes' runs part[0, nl), nl a power of two: step o = 1, 2, 4, ... joins lane + o onto every lane that is
// a multiple of 2 o; behind the step o = nl / 2 part[0] is the member's. A barrier stands between two steps.
ZZ_HD inline void zi_mpd_fold_step(zi_pr_part* part, uint32_t lane, uint32_t nl, uint32_t o)
{
    if ((lane & (2 * o - 1)) == 0 && lane + o < nl) part[lane] = zi_pr_join(ZI_CKS_CRC, part[lane], part[lane + o]);
}
// conditions 1, 3, 4 (and 2 through segs_ok) of member M of the file src[0, n): true iff it is proven. `all`: its segments' sums joined.
ZZ_HD inline bool zi_mpd_verdict(const uint8_t* src, uint64_t n, const zi_mpd_member& M, const zi_pr_part& all, bool segs_ok)
{
    if (!segs_ok || M.c > n || all.len != M.out) return false;
    const int64_t hl = zi_header(1, src + M.c, n - M.c);
    if (hl < 0 || (uint64_t)hl != M.first - M.c) return false;
    const uint64_t t0 = (M.end + 7) >> 3;
    if (t0 > n || n - t0 < 8) return false;
    const zi_view<const uint8_t> t{ src + t0, 8 };
    const uint32_t c = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t l = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    return c == all.v && l == (uint32_t)M.out;
}

}  // namespace zz
