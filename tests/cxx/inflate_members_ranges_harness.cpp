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
#define HARNESS_NAME "inflate_members_ranges_harness"
#include "harness_reads.h"

using namespace zz;

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

    // check
    bool index_bad = false;
    for (uint64_t j = 0; j < entries; ++j) if (zi_mr_entry_bad(idx, entries, j, src_len)) index_bad = true;
    if (index_bad) {
        reads_all_fail(nranges, out_lens, status);
        return ZI_RV_DATA;
    }
    // the rest is harness_reads.h's; per touched member: its descriptor, zi_item onto its slot
    std::vector<zi_tables> tables(1);
    host_lanes lanes{ 0 };
    return reads_through_index(idx, entries, nranges, firsts, nbytes, dsts, caps, out_lens, status, waves,
        [&](const zi_mr_tables& tab, uint64_t t, uint64_t t0, std::vector<uint8_t>& stage, unit_result* u) {
            const zi_mr_slot s = zi_mr_desc(tab, t, t0, src_len);
            const zi_view<const uint8_t> whole = view_of(src);
            if (s.src_len) (void)whole[s.src_off + s.src_len - 1];               // the member lies inside the source
            const std::vector<uint8_t> item(src.begin() + s.src_off, src.begin() + s.src_off + s.src_len);          // exactly its bytes
            const zi_view<uint8_t> st{ stage.data(), stage.size() };
            if (s.room) (void)st[s.stage_off + s.room - 1];                      // the slot lies inside the stage
            const zi_item_result r = zi_item(lanes, item.data(), s.src_len, stage.data() + s.stage_off, s.room, 1, tables[0], 0, 1);
            *u = unit_result{ r.status, r.status == ZI_ITEM_OK ? r.out : ~0ull, s.room };       // (what k_inflate_items stores)
            if (!(tab.tlist[t] & ZI_MR_BIG)) ++*members_decoded;
            return true;
        });
}
