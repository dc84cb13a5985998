"""Residency is what the device-side index builder rests on: one wavefront per chunk (k_points_find) and one per measured stretch
(k_points_reach) only pay when a CU holds sixteen of them, as it does of k_inflate_segments. Neither writes a decoded byte, so the
LDS holds the tables and the 2 KiB input stage -- the finder's tile shares that stage -- and nothing else: no more than
k_inflate_segments' 9,232 bytes; at most 128 VGPRs, nothing spilled, no scratch (CPU only: hipcc cross-compiles gfx950;
tools/scratch_report.py is the long form)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SEGMENTS = "_ZN2zz18k_inflate_segmentsENS_12zz_pt_paramsE"
KERNELS = ("_ZN2zz13k_points_findENS_12zz_pf_paramsE", "_ZN2zz14k_points_reachENS_12zz_pf_paramsE")
FINDER_STAGE = 0                                                   # the finder's tile IS the input stage: no bytes of its own


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


@pytest.mark.parametrize("name", KERNELS)
def test_sixteen_workgroups_on_a_cu(report, name):
    u = usage(report, name)
    lds = int(u["LDS Size [bytes/block]"])
    assert int(usage(report, SEGMENTS)["LDS Size [bytes/block]"]) == 9232
    assert lds <= 9232 + FINDER_STAGE, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"
    m = re.search(r"%s: (\d+) scratch_store, (\d+) scratch_load instructions" % re.escape(name), report)   # the long form
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0)
