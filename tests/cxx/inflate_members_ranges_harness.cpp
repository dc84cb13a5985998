// inflate_members_ranges_harness.cpp -- CPU harness of the rules of zz_decode_members_ranges_device
// (zzflate_amd/csrc/zz_inflate_core.h, zi_mr_*): a host restatement of the device's procedure -- index check, plan, differences,
// touched scan, waves, descriptors, zi_item per touched member onto a stage, F, cut, chunked copy, verdict -- with the very
// functions the kernels of zz_inflate_members_ranges.h call. tests/test_members_ranges_cases_cpu.py builds it with g++
// -DZZ_INFLATE_CHECKED (every access of the core and of this file's tables goes through a checked view; out of range aborts the
// process), once with the product's ZZ_MR_STAGE and once with a stage of a few hundred bytes, so that waves and big members
// occur in files of a few kilobytes.
//
//   zmr_reads(src, n, idx, entries, nranges, firsts, nbytes, dsts, caps, out_lens, status, &members_decoded, &waves) -> the call's code
//   zmr_stage() -> ZZ_MR_STAGE of this build
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zzflate_amd/csrc/zz_inflate_core.h"

using namespace zz;

namespace {

// zi_item's lane group with one lane
struct host_in {
    zi_view<const uint8_t> v;
    uint64_t peek8(uint64_t pos) const
    {
        uint64_t r = 0;
        for (uint32_t i = 0; i < 8; ++i) if (pos + i < v.n) r |= (uint64_t)v[pos + i] << (8 * i);
        return r;
    }
};
struct host_fence { void operator()() const {} };
struct host_lanes {
    typedef host_in in_t;
    typedef host_fence fence_t;
    in_t input(const uint8_t* p, uint64_t n) const { return in_t{ zi_view<const uint8_t>{ p, n } }; }
    void sync() const {}
    uint64_t sum(uint64_t v) const { return v; }
    uint32_t fold_xor(uint32_t v) const { return v; }
};

template <class T> zi_view<const T> view_of(const std::vector<T>& v) { return zi_view<const T>{ v.data(), v.size() }; }

}  // namespace

extern "C" uint64_t zmr_stage(void) { return ZZ_MR_STAGE; }

// the ABI's codes: 0 ok, -2 no space, -4 argument, -5 unsupported, -6 data
extern "C" int zmr_reads(const uint8_t* src_in, uint64_t src_len, const uint64_t* idx_in, uint64_t entries, uint64_t nranges,
                         const uint64_t* firsts, const uint64_t* nbytes, uint8_t* const* dsts, const uint64_t* caps,
                         uint64_t* out_lens, int32_t* status, uint64_t* members_decoded, uint32_t* waves)
{
    *members_decoded = 0; *waves = 0;
    if (!src_in || !idx_in || !firsts || !nbytes || !dsts || !caps || !out_lens) return ZI_RV_ARG;
    if (entries < 2 || entries - 1 > 0x7fffffffull || nranges > 0x7fffffffull) return ZI_RV_ARG;
    if (nranges == 0) return ZI_RV_OK;
    const std::vector<uint8_t> src(src_in, src_in + src_len);                     // exactly the file's bytes
    const std::vector<uint64_t> idxv(idx_in, idx_in + 2 * entries);               // exactly the index's words
    const zi_view<const uint64_t> idx = view_of(idxv);
    const uint64_t members = entries - 1;

    // check
    bool index_bad = false;
    for (uint64_t j = 0; j < entries; ++j) if (zi_mr_entry_bad(idx, entries, j, src_len)) index_bad = true;
    if (index_bad) {
        for (uint64_t r = 0; r < nranges; ++r) { out_lens[r] = ~0ull; if (status) status[r] = ZI_RV_DATA; }
        return ZI_RV_DATA;
    }
    // plan
    std::vector<zi_mr_read> reads(nranges);
    std::vector<int32_t> diff(entries, 0);
    for (uint64_t r = 0; r < nranges; ++r) {
        reads[r] = zi_mr_plan(idx, entries, firsts[r], nbytes[r], caps[r]);
        if (reads[r].any) { ++diff.at(reads[r].j0); --diff.at((uint64_t)reads[r].j1 + 1); }
    }
    // touched
    std::vector<uint32_t> cnt(entries, 0), tlist, G;
    std::vector<uint64_t> S;
    int64_t cov = 0; uint64_t room_sum = 0; uint32_t nbig = 0;
    for (uint64_t j = 0; j < members; ++j) {
        cov += diff[j];
        cnt[j] = (uint32_t)tlist.size();
        const uint64_t room = zi_mr_room(idx, j);
        const uint32_t kind = zi_mr_touch(room, cov > 0 ? 1 : 0);
        if (!kind) continue;
        tlist.push_back((uint32_t)j | (kind == 2 ? ZI_MR_BIG : 0u));
        S.push_back(room_sum); G.push_back(nbig);
        if (kind == 2) ++nbig; else room_sum += room;
    }
    const uint64_t T = tlist.size();
    cnt[members] = (uint32_t)T;
    S.push_back(room_sum); G.push_back(nbig);
    std::vector<uint32_t> F(T + 1, 0);
    const zi_mr_tables tab{ idx, view_of(cnt), view_of(tlist), view_of(S), view_of(F), view_of(G) };
    // waves
    if (T) {
        const uint64_t nwaves = zi_mr_wave(S[T - 1]) + 1;
        std::vector<uint64_t> first_rank(nwaves + 1, T);
        for (uint64_t w = 0; w < nwaves; ++w) first_rank[w] = zi_mr_wave_first(view_of(S), T, w * ZZ_MR_STAGE);
        zi_tables* tables = new zi_tables();
        host_lanes lanes;
        for (uint64_t w = 0; w < nwaves; ++w) {
            const uint64_t t0 = first_rank[w], t1 = first_rank[w + 1];
            if (t1 <= t0) continue;
            ++*waves;
            std::vector<uint8_t> stage(S[t1] - S[t0], 0xCD);                      // exactly the wave's rooms
            if (stage.size() >= 2 * ZZ_MR_STAGE) { fprintf(stderr, "inflate_members_ranges_harness: a wave of two stages\n"); abort(); }
            for (uint64_t t = t0; t < t1; ++t) {
                const zi_mr_slot s = zi_mr_desc(tab, t, t0, src_len);
                const zi_view<const uint8_t> whole = view_of(src);
                if (s.src_len) (void)whole[s.src_off + s.src_len - 1];           // the member lies inside the source
                const std::vector<uint8_t> item(src.begin() + s.src_off, src.begin() + s.src_off + s.src_len);      // exactly its bytes
                const zi_view<uint8_t> st{ stage.data(), stage.size() };
                if (s.room) (void)st[s.stage_off + s.room - 1];                  // the slot lies inside the stage
                const zi_item_result r = zi_item(lanes, item.data(), s.src_len, stage.data() + s.stage_off, s.room, 1, *tables, 0, 1);
                const uint64_t out = r.status == ZI_ITEM_OK ? r.out : ~0ull;     // (what k_inflate_items stores)
                F[t + 1] = F[t] + (zi_mr_member_bad(tlist[t], r.status, out, s.room) ? 1u : 0u);
                if (!(tlist[t] & ZI_MR_BIG)) ++*members_decoded;
            }
            // cut and copy, chunk by chunk
            for (uint64_t r = 0; r < nranges; ++r) {
                const zi_mr_piece p = zi_mr_cut(reads[r], firsts[r], tab, t0, t1);
                const uint64_t room = reads[r].m < caps[r] ? reads[r].m : caps[r];
                const zi_view<uint8_t> d{ dsts[r], room };
                const zi_view<const uint8_t> st{ stage.data(), stage.size() };
                for (uint64_t k = 0; k < zi_mr_chunks(p.len); ++k) {
                    const uint64_t at = k * ZZ_MR_CHUNK, n = p.len - at < ZZ_MR_CHUNK ? p.len - at : ZZ_MR_CHUNK;
                    for (uint64_t i = 0; i < n; ++i) d[p.dst_off + at + i] = st[p.stage_off + at + i];
                }
            }
        }
        delete tables;
    }
    // verdict
    uint64_t n_data = 0, n_unsupported = 0, n_arg = 0, n_nospace = 0;
    for (uint64_t r = 0; r < nranges; ++r) {
        const int v = zi_mr_verdict(reads[r], tab);
        out_lens[r] = v == ZI_RV_OK ? reads[r].m : ~0ull;
        if (status) status[r] = v;
        n_data += v == ZI_RV_DATA; n_unsupported += v == ZI_RV_UNSUPPORTED; n_arg += v == ZI_RV_ARG; n_nospace += v == ZI_RV_NOSPACE;
    }
    return n_data ? ZI_RV_DATA : n_unsupported ? ZI_RV_UNSUPPORTED : n_arg ? ZI_RV_ARG : n_nospace ? ZI_RV_NOSPACE : ZI_RV_OK;
}
