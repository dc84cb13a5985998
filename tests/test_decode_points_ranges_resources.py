"""What the kernels of zz_decode_points_ranges_device cost a CU, from the numbers of the compiler's resource report alone
(tools/scratch_report.py; CPU only: hipcc cross-compiles gfx950). k_inflate_segments_win has k_inflate_segments' budget -- its
window is read where it lies in global memory, so the LDS holds the tables and the input stage and nothing else: at most 10,240
bytes per workgroup (sixteen in a CU's 160 KiB), at most 128 VGPRs, no vector register spilled, no scratch, no dynamic stack
(scalar registers the compiler parks in vector lanes cost neither). And the kernels this call shares or stands beside --
k_inflate_segments, k_inflate_items and the k_mr_* kernels -- report what they reported before this call existed: the numbers
below are the parent commit's (VGPRs, SGPRs, LDS bytes, scratch bytes, VGPR spills, SGPR spills). k_mr_touched's are those it
has had since its three scans became calls of wg_scan_excl (zz_wave.h): 95 vector registers where it had 102, 100 scalar ones where
it had 84 -- five wavefronts a SIMD where it had four, LDS, scratch and spills as before."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
WIN = "_ZN2zz22k_inflate_segments_winENS_12zz_mr_paramsENS_12zz_pr_paramsEmm"
FRONT = "_ZN2zz10k_pr_frontENS_12zz_mr_paramsENS_12zz_pr_paramsE"
BEFORE = {
    "_ZN2zz15k_inflate_itemsENS_19zz_inf_items_paramsE": (117, 106, 9232, 0, 0, 38),
    "_ZN2zz18k_inflate_segmentsENS_12zz_pt_paramsE": (99, 106, 9232, 0, 0, 4),
    "_ZN2zz10k_mr_checkENS_12zz_mr_paramsE": (10, 36, 0, 0, 0, 0),
    "_ZN2zz9k_mr_planENS_12zz_mr_paramsE": (24, 59, 0, 0, 0, 0),
    "_ZN2zz12k_mr_touchedENS_12zz_mr_paramsE": (95, 100, 256, 0, 0, 0),
    "_ZN2zz10k_mr_wavesENS_12zz_mr_paramsEmPm": (14, 24, 0, 0, 0, 0),
    "_ZN2zz9k_mr_descENS_12zz_mr_paramsEmmPPKhPmPPhS4_": (24, 44, 0, 0, 0, 0),
    "_ZN2zz10k_mr_judgeENS_12zz_mr_paramsEmmPKmS2_PKi": (48, 56, 64, 0, 0, 0),
    "_ZN2zz8k_mr_cutENS_12zz_mr_paramsEmm": (76, 94, 128, 0, 0, 0),
    "_ZN2zz9k_mr_copyENS_12zz_mr_paramsEmm": (48, 78, 0, 0, 0, 0),
    "_ZN2zz12k_mr_verdictENS_12zz_mr_paramsE": (22, 46, 0, 0, 0, 0),
}


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for m in re.finditer(r"Function Name: (\S+)\n((?:    .*\n)+)", r.stdout):
        out[m.group(1)] = {k.strip(): v.strip() for k, v in (ln.split(":", 1) for ln in m.group(2).splitlines())}
    return out


def test_window_kernel_keeps_sixteen_workgroups_on_a_cu(usage):
    u = usage[WIN]
    lds = int(u["LDS Size [bytes/block]"])
    assert lds <= 10240, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"


def test_front_kernel_is_one_plain_workgroup(usage):
    u = usage[FRONT]
    assert int(u["VGPRs"]) <= 64 and int(u["LDS Size [bytes/block]"]) <= 16384      # 1,024 lanes need at most 64 registers each
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"


@pytest.mark.parametrize("kernel", sorted(BEFORE))
def test_the_neighbours_report_what_they_reported(usage, kernel):
    u = usage[kernel]
    now = (int(u["VGPRs"]), int(u["TotalSGPRs"]), int(u["LDS Size [bytes/block]"]), int(u["ScratchSize [bytes/lane]"]),
           int(u["VGPRs Spill"]), int(u["SGPRs Spill"]))
    assert now == BEFORE[kernel]
    assert u["Dynamic Stack"] == "False"
