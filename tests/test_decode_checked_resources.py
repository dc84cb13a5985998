"""The checked range reads add kernels beside the range decode's and leave its own alone: the new ones (zz_inflate_check.h) use no
scratch and spill nothing, and phase 1 and the rounds of the single and the multi read -- the bodies both the checked and the
unchecked calls run -- keep exactly the registers, LDS and scratch the commit before the checked reads compiled them to (CPU only:
hipcc cross-compiles gfx950; tools/scratch_report.py is the long form)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
# VGPRs, LDS bytes per block, scratch bytes per lane as the commit before zz_inflate_check.h compiled them (ROCm 7.2, gfx950)
BEFORE = {
    "_ZN2zz23k_inflate_packets_rangeENS_13zz_inf_paramsE": (109, 7184, 0),
    "_ZN2zz24k_inflate_packets_rangesENS_13zz_inf_paramsENS_13zz_inf_rangesE": (109, 7184, 0),
    "_ZN2zz23k_inflate_resolve_rangeENS_13zz_res_paramsENS_12zz_res_rangeEj": (25, 16, 0),
    "_ZN2zz24k_inflate_resolve_rangesENS_13zz_res_paramsENS_13zz_inf_rangesEj": (28, 16, 0),
}
NEW = [
    "_ZN2zz13k_adler_stageE16zz_packet_paramsNS_12zz_stage_mapE",
    "_ZN2zz13k_crc32_stageE16zz_packet_paramsNS_12zz_stage_mapE",
    "_ZN2zz13k_cks_publishEPK6zz_cksjjmiPj",
    "_ZN2zz16k_sidecar_unpackEPKjjjmiP6zz_cksPj",
    "_ZN2zz17k_sidecar_verdictEPKhiPKNS_12zz_cks_totalEmPj",
    "_ZN2zz19k_stage_check_rangeENS_13zz_chk_paramsEmjPy",
    "_ZN2zz20k_stage_check_rangesENS_13zz_chk_paramsEPKNS_12zi_read_descEjPNS_7zi_readE",
]


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


def test_the_new_kernels_use_no_scratch_and_spill_nothing(report):
    for name in NEW:
        u = usage(report, name)
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and u["Dynamic Stack"] == "False", name
        assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, name


def test_the_stage_crc_kernel_is_the_packet_kernels_body(report):
    """the stage form of the CRC-32 pass is the same body behind another packet view: the same two tables in the LDS"""
    a = usage(report, "_ZN2zz15k_crc32_packetsE16zz_packet_params")
    b = usage(report, "_ZN2zz13k_crc32_stageE16zz_packet_paramsNS_12zz_stage_mapE")
    assert a["LDS Size [bytes/block]"] == b["LDS Size [bytes/block]"] == "8208"


def test_phase_one_and_the_rounds_are_what_they_were(report):
    for name, want in BEFORE.items():
        u = usage(report, name)
        assert (int(u["VGPRs"]), int(u["LDS Size [bytes/block]"]), int(u["ScratchSize [bytes/lane]"])) == want, name
