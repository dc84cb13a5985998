"""What the new passes of zz_encode_members_device cost a CU (CPU only: hipcc cross-compiles gfx950): bookkeeping and bandwidth
passes, so none of them spills or uses scratch, and the per-packet and per-member ones keep full occupancy. The test compiles a
translation unit of its own that holds zz_members_write.h and what it includes; the packet kernels the call launches are the
batch's, held to their budgets by tests/test_batch_resources.py."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["k_mw_items", "k_mw_desc", "k_mw_sizes", "k_mw_finalize", "k_mw_compact", "k_mw_stored"]
PER_PACKET_OR_MEMBER = ["k_mw_items", "k_mw_desc", "k_mw_finalize", "k_mw_compact", "k_mw_stored"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    d = tmp_path_factory.mktemp("members_write_resources")
    src = d / "members_write.hip"
    header = os.path.join(ROOT, "zzflate_amd", "csrc", "zz_members_write.h")
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s"\n' % header)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(d / "members_write.s"), str(src)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = out.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return out


def find(usage, part):
    hits = [v for k, v in usage.items() if part in k]
    assert len(hits) == 1, (part, sorted(usage))
    return hits[0]


@pytest.mark.parametrize("kernel", NEW)
def test_no_scratch_and_no_spills(usage, kernel):
    u = find(usage, kernel)
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["SGPRs Spill"]) == 0
    assert u["Dynamic Stack"] == "False"


@pytest.mark.parametrize("kernel", PER_PACKET_OR_MEMBER)
def test_per_packet_and_per_member_passes_keep_full_occupancy(usage, kernel):
    assert int(find(usage, kernel)["VGPRs"]) <= 64, kernel


def test_the_scan_needs_next_to_no_lds(usage):
    assert int(find(usage, "k_mw_sizes")["LDS Size [bytes/block]"]) <= 128
