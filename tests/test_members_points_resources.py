"""Residency of the member point index's kernel. k_members_points_reach measures one job per wavefront and only pays when a CU holds
sixteen of them, as it does of k_points_reach: nothing is written, so the LDS holds the tables and the 2 KiB input stage and nothing
else -- no more than k_inflate_segments' 9,232 bytes -- with at most 128 VGPRs, nothing spilled, no scratch: the conditions
tests/test_points_index_resources.py sets (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
from test_members_find_resources import no_scratch
from test_points_index_resources import SEGMENTS, report, usage  # noqa: F401  (the module-scoped report fixture)

REACH = "_ZN2zz22k_members_points_reachENS_12zz_mp_paramsE"


def test_sixteen_reach_workgroups_on_a_cu(report):
    u = no_scratch(report, REACH)
    lds = int(u["LDS Size [bytes/block]"])
    assert int(usage(report, SEGMENTS)["LDS Size [bytes/block]"]) == 9232
    assert lds <= 9232, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]


def test_the_kernels_this_is_made_of_are_what_they_were(report):
    """the unchanged kernels in front of the new one: present under their names, at k_inflate_segments' figure"""
    for name in ("_ZN2zz13k_points_findENS_12zz_pf_paramsE", "_ZN2zz14k_points_reachENS_12zz_pf_paramsE",
                 "_ZN2zz15k_members_reachENS_12zz_mf_paramsE", SEGMENTS):
        assert int(usage(report, name)["LDS Size [bytes/block]"]) == 9232, name
