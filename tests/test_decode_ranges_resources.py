"""Phase 1's residency is three workgroups per CU: a 32 KiB packet's dynamic LDS (4,096 bytes of bitmap, 2,048 of staged input,
the 32,768-byte window) beside the static tables, three times in a CU's 160 KiB. The multi-range decode's third form of the
phase-1 kernel keeps to that -- no scratch, nothing spilled, at most 128 VGPRs -- and the single read's kernels it shares the
bodies with are what they were (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
RANGES = "_ZN2zz24k_inflate_packets_rangesENS_13zz_inf_paramsENS_13zz_inf_rangesE"
# VGPRs, LDS bytes per block, scratch bytes per lane as the commit before k_inflate_packets_ranges compiled them (ROCm 7.2, gfx950)
BEFORE = {
    "_ZN2zz23k_inflate_packets_rangeENS_13zz_inf_paramsE": (109, 7184, 0),
    "_ZN2zz23k_inflate_resolve_rangeENS_13zz_res_paramsENS_12zz_res_rangeEj": (25, 16, 0),
}


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def usage(report, mangled):
    m = re.search(r"Function Name: %s\n(.*?)\n\n" % re.escape(mangled), report, flags=re.S)
    assert m, mangled
    return {k.strip(): v.strip() for k, v in (ln.split(":", 1) for ln in m.group(1).splitlines() if ":" in ln)}


def test_ranges_phase_one_keeps_three_workgroups_on_a_cu(report):
    u = usage(report, RANGES)
    lds = int(u["LDS Size [bytes/block]"]) + 4096 + 2048 + 32768
    assert -(-lds // 512) * 512 * 3 <= 160 * 1024, lds            # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"


def test_the_single_read_kernels_are_what_they_were(report):
    for name, want in BEFORE.items():
        u = usage(report, name)
        assert (int(u["VGPRs"]), int(u["LDS Size [bytes/block]"]), int(u["ScratchSize [bytes/lane]"])) == want, name
