"""Residency of the member finder's kernels. k_members_reach measures one candidate per wavefront and only pays when a CU holds
sixteen of them, as it does of k_points_reach: nothing is written, so the LDS holds the tables and the 2 KiB input stage and nothing
else -- no more than k_inflate_segments' 9,232 bytes -- with at most 128 VGPRs, nothing spilled, no scratch: the conditions
tests/test_points_index_resources.py sets. The mark pass is a bandwidth pass and the slots kernel one workgroup: a few words of
LDS for their scans, no scratch (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
import re

import pytest

from test_points_index_resources import SEGMENTS, report, usage  # noqa: F401  (the module-scoped report fixture)

REACH = "_ZN2zz15k_members_reachENS_12zz_mf_paramsE"
MARKS = ("_ZN2zz19k_members_find_markILb0EEEvPKhmPjPKmPm", "_ZN2zz19k_members_find_markILb1EEEvPKhmPjPKmPm")
SLOTS = "_ZN2zz20k_members_find_slotsENS_11zz_mf_slotsE"


def no_scratch(report, name):
    u = usage(report, name)
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"
    m = re.search(r"%s: (\d+) scratch_store, (\d+) scratch_load instructions" % re.escape(name), report)   # the long form
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0)
    return u


def test_sixteen_reach_workgroups_on_a_cu(report):
    u = no_scratch(report, REACH)
    lds = int(u["LDS Size [bytes/block]"])
    assert int(usage(report, SEGMENTS)["LDS Size [bytes/block]"]) == 9232
    assert lds <= 9232, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]


@pytest.mark.parametrize("name", MARKS)
def test_the_mark_pass_is_k_members_marks_size(report, name):
    u = no_scratch(report, name)
    twin = usage(report, name.replace("19k_members_find_mark", "14k_members_mark").replace("PKmPm", "PKmPmS3_"))
    assert int(u["LDS Size [bytes/block]"]) == int(twin["LDS Size [bytes/block]"]) == 16    # one word per wavefront for the scan
    assert int(u["VGPRs"]) <= 64, "eight workgroups of 256 threads on a CU"


def test_the_slots_kernel(report):
    u = no_scratch(report, SLOTS)
    assert int(u["LDS Size [bytes/block]"]) == 16 * 4 + 16 * 8    # the two scans' wavefront totals
    assert int(u["VGPRs"]) <= 128
