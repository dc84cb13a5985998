// harness_reads.h -- the host restatement of the reads through an index (the zi_mr_* rules of zzflate_amd/csrc/zz_inflate_core.h),
// shared by inflate_members_ranges_harness.cpp and inflate_points_ranges_harness.cpp as the device's two calls share their
// kernels: plan, differences, touched scan, tables, waves, one callback per touched rank, F, cut, chunked copy, verdict and the
// call's code. Index check and front are the including file's: they differ. Every table goes through a checked view.
#pragma once
#include "harness_lanes.h"

// what the check (or a front) does when it refuses the index: every read fails
inline void reads_all_fail(uint64_t nranges, uint64_t* out_lens, int32_t* status)
{
    for (uint64_t r = 0; r < nranges; ++r) { out_lens[r] = ~0ull; if (status) status[r] = zz::ZI_RV_DATA; }
}

// what a unit's decode left: k_inflate_items' words (out = ~0 unless the status is ZI_ITEM_OK) and the unit's room
struct unit_result { int status; uint64_t out, room; };

// unit(tab, t, t0, stage, &result) -> false: a harness failure (the call answers -100). It decodes the touched rank t of the
// wave that begins at rank t0 onto its slot of `stage`, which is exactly the wave's rooms.
template <class Unit>
int reads_through_index(const zz::zi_view<const uint64_t>& idx, uint64_t entries, uint64_t nranges, const uint64_t* firsts,
                        const uint64_t* nbytes, uint8_t* const* dsts, const uint64_t* caps, uint64_t* out_lens, int32_t* status,
                        uint32_t* waves, Unit unit)
{
    using namespace zz;
    const uint64_t units = entries - 1;
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
    for (uint64_t j = 0; j < units; ++j) {
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
    cnt[units] = (uint32_t)T;
    S.push_back(room_sum); G.push_back(nbig);
    std::vector<uint32_t> F(T + 1, 0);
    const zi_mr_tables tab{ idx, view_of(cnt), view_of(tlist), view_of(S), view_of(F), view_of(G) };
    // waves
    if (T) {
        const uint64_t nwaves = zi_mr_wave(S[T - 1]) + 1;
        std::vector<uint64_t> first_rank(nwaves + 1, T);
        for (uint64_t w = 0; w < nwaves; ++w) first_rank[w] = zi_mr_wave_first(view_of(S), T, w * ZZ_MR_STAGE);
        for (uint64_t w = 0; w < nwaves; ++w) {
            const uint64_t t0 = first_rank[w], t1 = first_rank[w + 1];
            if (t1 <= t0) continue;
            ++*waves;
            std::vector<uint8_t> stage(S[t1] - S[t0], 0xCD);                      // exactly the wave's rooms
            if (stage.size() >= 2 * ZZ_MR_STAGE) { fprintf(stderr, HARNESS_NAME ": a wave of two stages\n"); abort(); }
            for (uint64_t t = t0; t < t1; ++t) {
                unit_result u{ ZI_ITEM_DATA, ~0ull, 0 };
                if (!unit(tab, t, t0, stage, &u)) return -100;
                F[t + 1] = F[t] + (zi_mr_member_bad(tlist[t], u.status, u.out, u.room) ? 1u : 0u);
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
