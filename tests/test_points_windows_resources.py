"""k_points_windows_cut has k_inflate_segments' shape -- one wavefront per workgroup, persistent -- so what it may cost is what lets
sixteen of them stay on a CU beside each other: no scratch, no spills, an LDS share that fits sixteen times (it uses none), and
the registers the code object reports, pinned here as the sibling tests pin theirs. The three decode kernels the builder launches
unchanged -- k_inflate_segments, k_points_count, k_inflate_resolve -- report what they reported before the builder existed (CPU
only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CUT = "_ZN2zz20k_points_windows_cutENS_12zz_pw_paramsE"
# (VGPRs, LDS bytes per block, waves per SIMD) of the kernels the builder shares with zz_decode_points_device
UNCHANGED = {
    "_ZN2zz18k_inflate_segmentsENS_12zz_pt_paramsE": (99, 9232, 4),
    "_ZN2zz14k_points_countEPKjPjS2_Py": (8, 16, 8),
    "_ZN2zz17k_inflate_resolveENS_13zz_res_paramsEj": (24, 16, 8),
}


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def usage(report, name):
    m = re.search(r"Function Name: %s\n(.*?)\n\n" % re.escape(name), report, flags=re.S)
    assert m, name
    return {k.strip(): v.strip() for k, v in (ln.split(":", 1) for ln in m.group(1).splitlines() if ":" in ln)}


def test_the_cut_kernel_keeps_sixteen_workgroups_on_a_cu(report):
    u = usage(report, CUT)
    lds = int(u["LDS Size [bytes/block]"])
    assert lds == 0, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) == 25, u["VGPRs"]
    assert int(u["VGPRs"]) <= 128                                 # four wavefronts per SIMD: sixteen workgroups of one wavefront per CU
    assert int(u["Occupancy [waves/SIMD]"]) >= 4
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"
    m = re.search(r"k_points_windows_cutE\w*: (\d+) scratch_store, (\d+) scratch_load instructions", report)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0)


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_the_shared_decode_kernels_report_what_they_did(report, name):
    u = usage(report, name)
    assert (int(u["VGPRs"]), int(u["LDS Size [bytes/block]"]), int(u["Occupancy [waves/SIMD]"])) == UNCHANGED[name], name
    assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0
