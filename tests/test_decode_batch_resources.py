"""Residency is the point of the batch decoder's kernel: one wavefront per stream only pays when a CU holds many of them. So
k_inflate_items keeps to sixteen workgroups per CU -- at most 10,240 bytes of LDS per workgroup (sixteen in a CU's 160 KiB)
and at most 128 VGPRs (four wavefronts per SIMD), nothing spilled, no scratch -- and the decode kernels it shares the core with
are what they were (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
ITEMS = "_ZN2zz15k_inflate_itemsENS_19zz_inf_items_paramsE"
# VGPRs, LDS bytes per block, scratch bytes per lane of the kernels that share zz_inflate_core.h, as the commit before
# k_inflate_items compiled them (ROCm 7.2, gfx950)
BEFORE = {
    "_ZN2zz16k_inflate_serialEPKhmPhmPNS_17zz_inf_serial_outE": (83, 9232, 0),
    "_ZN2zz17k_inflate_packetsENS_13zz_inf_paramsE": (109, 7184, 0),
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


def test_item_kernel_keeps_sixteen_workgroups_on_a_cu(report):
    u = usage(report, ITEMS)
    lds = int(u["LDS Size [bytes/block]"])
    assert lds <= 10240, lds
    assert -(-lds // 512) * 512 * 16 <= 160 * 1024, lds           # the LDS is handed out in 512-byte steps
    assert int(u["VGPRs"]) <= 128, u["VGPRs"]
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert u["Dynamic Stack"] == "False"
    # the long form lists its scratch accesses: none
    m = re.search(r"k_inflate_itemsE\w*: (\d+) scratch_store, (\d+) scratch_load instructions", report)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0)


def test_the_other_decode_kernels_are_what_they_were(report):
    for name, want in BEFORE.items():
        u = usage(report, name)
        assert (int(u["VGPRs"]), int(u["LDS Size [bytes/block]"]), int(u["ScratchSize [bytes/lane]"])) == want, name
