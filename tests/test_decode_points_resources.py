"""Residency is the point of the segment kernel, as it is of the batch decoder's: one wavefront per segment only pays when a CU
holds many of them. k_inflate_segments decodes onto the destination, so its LDS holds the tables and the input stage and nothing
else: at most 10,240 bytes per workgroup (sixteen in a CU's 160 KiB), at most 128 VGPRs (four wavefronts per SIMD), nothing
spilled, no scratch (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form). The other decode kernels
are judged by the resource tests that were there before."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SEGMENTS = "_ZN2zz18k_inflate_segmentsENS_12zz_pt_paramsE"


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_segment_kernel_keeps_sixteen_workgroups_on_a_cu(report):
    m = re.search(r"Function Name: %s\n(.*?)\n\n" % re.escape(SEGMENTS), report, flags=re.S)
    assert m, SEGMENTS
    u = {k.strip(): v.strip() for k, v in (ln.split(":", 1) for ln in m.group(1).splitlines() if ":" in ln)}
    lds = int(u["LDS Size [bytes/block]"])
    assert lds <= 10240, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"
    # the long form lists its scratch accesses: none
    m = re.search(r"k_inflate_segmentsE\w*: (\d+) scratch_store, (\d+) scratch_load instructions", report)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0)
