"""The batch forms of the extended levels' two kernels keep their single forms' budgets -- a CU to itself for k_l6_matches_batch,
eleven workgroups per CU for the batch XD encode kernel -- and the single forms are held to the resource lines the commit before
the batch forms gave them (CPU only: hipcc cross-compiles gfx950; tools/scratch_report.py is the long form).

The pin of the single forms (ROCm 7.2, gfx950; VGPRs, TotalSGPRs, LDS bytes, scratch bytes per lane) is what the commit before
compiled them to, with the body in the kernel itself. Behind l6_matches_run<DEPTH, MAP> the register allocator is sensitive to how
the body receives its parameters and its packet view (a view by reference gave 73 / 73 / 73 or 75 / 75 / 75 VGPRs for depths
2 / 4 / 8); with the parameters and the packet's view by value the three kernels compile to the pinned 75 / 75 / 73."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"

# the single-stream kernels of the extended levels as the commit before the batch forms compiled them
BEFORE = {
    "_ZN2zz12k_l6_matchesILi2EEEvNS_13zz_l6m_paramsE": (75, 106, 163032, 0),
    "_ZN2zz12k_l6_matchesILi4EEEvNS_13zz_l6m_paramsE": (75, 106, 163032, 0),
    "_ZN2zz12k_l6_matchesILi8EEEvNS_13zz_l6m_paramsE": (73, 106, 163032, 0),
    "_ZN2zz13k_encode_l2_tILj32768ELb1ELb0EEEvNS_12zz_l2_paramsE": (80, 106, 13760, 16),
}
MATCHES_BATCH = "_ZN2zz18k_l6_matches_batchILi%dEEEvNS_13zz_l6m_paramsE12zz_batch_map"
ENCODE_BATCH = "_ZN2zz18k_encode_l2x_batchENS_12zz_l2_paramsE12zz_batch_map"


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


def line(u):
    return (int(u["VGPRs"]), int(u["TotalSGPRs"]), int(u["LDS Size [bytes/block]"]), int(u["ScratchSize [bytes/lane]"]))


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_single_stream_kernels_are_unchanged(report, name):
    got = line(usage(report, name))
    print(name, "before", BEFORE[name], "now", got)
    assert got == BEFORE[name]


@pytest.mark.parametrize("depth", [2, 4, 8])
def test_the_batch_match_kernel_owns_a_cu_without_spills(report, depth):
    u = usage(report, MATCHES_BATCH % depth)
    lds = int(u["LDS Size [bytes/block]"])
    assert 128 * 1024 < lds <= 160 * 1024, lds
    assert int(u["VGPRs"]) <= 128                                           # 16 wavefronts of one workgroup: four per SIMD
    assert int(u["VGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0


def test_the_batch_encode_kernel_fits_eleven_workgroups(report):
    u = usage(report, ENCODE_BATCH)
    lds = int(u["LDS Size [bytes/block]"])
    assert -(-lds // 512) * 512 * 11 <= 160 * 1024, lds
    assert int(u["VGPRs"]) <= 80                                            # 22 wavefronts per CU: six on two of the SIMDs
