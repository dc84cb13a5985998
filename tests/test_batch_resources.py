"""The batch forms of the packet kernels keep their single forms' budgets, and the single forms themselves are untouched by the
batch work: their resource lines are pinned to what they were before the batch forms existed (CPU only: hipcc cross-compiles
gfx950; tools/scratch_report.py is the long form)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"

# The resource lines of the single-stream encode kernels as the commit before the batch forms compiled them (ROCm 7.2, gfx950):
# VGPRs, TotalSGPRs, LDS bytes per block, scratch bytes per lane.
BEFORE = {
    "_ZN2zz12k_encode_l1pE16zz_packet_params": (62, 70, 17876, 0),
    "_ZN2zz11k_encode_l1E16zz_packet_params": (58, 105, 17408, 0),
    "_ZN2zz13k_encode_l2_tILj0ELb0ELb1EEEvNS_12zz_l2_paramsE": (72, 94, 17888, 144),
    "_ZN2zz13k_encode_l2_tILj0ELb0ELb0EEEvNS_12zz_l2_paramsE": (96, 106, 17856, 8),
    "_ZN2zz11k_encode_l0ENS_12zz_l0_paramsE": (103, 82, 64, 0),
}
L1P = "_ZN2zz18k_encode_l1p_batchE16zz_packet_params12zz_batch_map"
L1 = "_ZN2zz17k_encode_l1_batchE16zz_packet_params12zz_batch_map"
L2P = "_ZN2zz19k_encode_l2_batch_tILb1EEEvNS_12zz_l2_paramsE12zz_batch_map"
L2 = "_ZN2zz19k_encode_l2_batch_tILb0EEEvNS_12zz_l2_paramsE12zz_batch_map"
L0 = "_ZN2zz17k_encode_l0_batchENS_18zz_l0_batch_paramsE12zz_batch_map"
CRC = "_ZN2zz21k_crc32_packets_batchE16zz_packet_params12zz_batch_map"


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


def scratch_by_depth(report, mangled):
    short = mangled[len("_ZN2zz"):]
    m = re.search(r"%s: (\d+) scratch_store, (\d+) scratch_load instructions\n((?:  depth .*\n)*)" % re.escape(short), report)
    assert m, mangled
    return [(int(d), kind, int(c)) for d, c, kind in re.findall(r"depth (\d+):\s+(\d+) scratch_(store|load)", m.group(3))]


def test_single_stream_kernels_are_unchanged(report):
    for name, want in BEFORE.items():
        assert line(usage(report, name)) == want, name


def test_every_batch_kernel_exists(report):
    for name in (L0, L1, L1P, L2, L2P, CRC, "_ZN2zz12k_batch_planEPKmjjiPjPmPNS_15zz_batch_totalsE",
                 "_ZN2zz16k_batch_finalizeENS_13zz_batch_joinE", "_ZN2zz15k_batch_compactENS_13zz_batch_joinE"):
        usage(report, name)


def test_two_parser_level1_batch_kernel_keeps_nine_workgroups_of_three_wavefronts(report):
    u = usage(report, L1P)
    lds = int(u["LDS Size [bytes/block]"])
    assert -(-lds // 512) * 512 * 9 <= 160 * 1024, lds
    assert int(u["VGPRs"]) <= 72 and int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0
    assert scratch_by_depth(report, L1P) == []


def test_one_parser_level1_batch_kernel_fits_nine_workgroups_without_scratch(report):
    u = usage(report, L1)
    assert int(u["LDS Size [bytes/block]"]) * 9 <= 160 * 1024
    assert int(u["VGPRs"]) <= 96 and int(u["ScratchSize [bytes/lane]"]) == 0


def test_two_parser_level2_batch_kernel_fits_and_stores_no_scratch_in_the_block_loops(report):
    u = usage(report, L2P)
    lds = int(u["LDS Size [bytes/block]"])
    assert -(-lds // 512) * 512 * 9 <= 160 * 1024, lds
    assert int(u["VGPRs"]) <= 72
    stores = [d for d, kind, _ in scratch_by_depth(report, L2P) if kind == "store"]
    assert not stores or max(stores) <= 1, stores


def test_one_parser_level2_batch_kernel_fits_and_stores_no_scratch_in_the_block_loops(report):
    u = usage(report, L2)
    assert int(u["LDS Size [bytes/block]"]) * 9 <= 160 * 1024 and int(u["VGPRs"]) <= 96
    stores = [d for d, kind, _ in scratch_by_depth(report, L2) if kind == "store"]
    assert not stores or max(stores) <= 1, stores
