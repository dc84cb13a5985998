"""Residency of the decode through a member point index. Its phase 1, k_members_segments, is k_inflate_segments with a descriptor
per segment and only pays when a CU holds sixteen of its wavefronts: the window is the destination, so the LDS holds the tables and
the 2 KiB input stage and nothing else -- no more than k_inflate_segments' 9,232 bytes -- with at most 128 VGPRs, nothing spilled,
no scratch. The sums and the verdict stage nothing and must stay far below that; the kernels the call launches unchanged are at
the figures they had (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
from test_members_find_resources import no_scratch
from test_points_index_resources import SEGMENTS, report, usage  # noqa: F401  (the module-scoped report fixture)

PHASE1 = "_ZN2zz18k_members_segmentsENS_13zz_mpd_paramsE"
SUMS = "_ZN2zz14k_members_sumsENS_13zz_mpd_paramsE"
VERDICT = "_ZN2zz17k_members_verdictENS_21zz_mpd_verdict_paramsE"
# (LDS bytes per block, VGPRs) of the kernels launched unchanged, as they were in front of this call
UNCHANGED = {
    SEGMENTS: (9232, 99),
    "_ZN2zz14k_points_countEPKjPjS2_Py": (16, 8),
    "_ZN2zz17k_inflate_resolveENS_13zz_res_paramsEj": (16, 24),
    "_ZN2zz15k_inflate_itemsENS_19zz_inf_items_paramsE": (9232, 117),
    "_ZN2zz17k_inflate_membersEPKhmPhmPNS_18zz_inf_members_outE": (9232, 124),
}


def test_sixteen_phase_one_workgroups_on_a_cu(report):
    u = no_scratch(report, PHASE1)
    lds = int(u["LDS Size [bytes/block]"])
    assert lds <= 9232, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]


def test_sums_and_verdict_stage_nothing(report):
    for name, most in ((SUMS, 0), (VERDICT, 64 * 16)):            # the verdict's tree: one 16-byte partial per lane
        u = no_scratch(report, name)
        assert int(u["LDS Size [bytes/block]"]) <= most, name
        assert int(u["VGPRs"]) <= 128, name


def test_the_unchanged_kernels_are_at_their_old_figures(report):
    for name, (lds, vgprs) in UNCHANGED.items():
        u = usage(report, name)
        assert (int(u["LDS Size [bytes/block]"]), int(u["VGPRs"])) == (lds, vgprs), name
        assert int(u["ScratchSize [bytes/lane]"]) == 0, name
