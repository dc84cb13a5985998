"""What the kernels of zz_decode_members_ranges_device and zz_members_index_device cost a CU (CPU only: hipcc cross-compiles
gfx950): none of them spills, uses scratch or has a dynamic stack; the plan, check and verdict kernels and the copy kernel -- a
bandwidth pass -- keep full occupancy (at most 64 VGPRs at 256 lanes a workgroup), the copy with next to no LDS; and
k_inflate_items, which decodes the touched members unchanged, reports in this translation unit -- zz_inflate_members_ranges.h
and what it includes -- exactly what it reports in the product's (tools/scratch_report.py, test_decode_batch_resources.py's
build)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["k_mr_check", "k_mr_plan", "k_mr_touched", "k_mr_waves", "k_mr_desc", "k_mr_judge", "k_mr_cut", "k_mr_copy", "k_mr_verdict",
       "k_members_pairs"]
ITEMS = "_ZN2zz15k_inflate_itemsENS_19zz_inf_items_paramsE"
FIELDS = ("VGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Dynamic Stack", "Occupancy [waves/SIMD]")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    d = tmp_path_factory.mktemp("members_ranges_resources")
    src = d / "members_ranges.hip"
    csrc = os.path.join(ROOT, "zzflate_amd", "csrc")
    header = (os.path.join(csrc, "zz_checksum.h"), os.path.join(csrc, "zz_inflate_members_ranges.h"))      # (in zz_api.hip's order)
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s"\n#include "%s"\n' % header)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(d / "members_ranges.s"), str(src)], capture_output=True, text=True, timeout=900)
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
def test_no_scratch_no_spills_no_dynamic_stack(usage, kernel):
    u = find(usage, kernel)
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["SGPRs Spill"]) == 0
    assert u["Dynamic Stack"] == "False"


@pytest.mark.parametrize("kernel", ["k_mr_check", "k_mr_plan", "k_mr_verdict", "k_mr_copy"])
def test_light_kernels_keep_full_occupancy(usage, kernel):
    u = find(usage, kernel)
    assert int(u["VGPRs"]) <= 64, (kernel, u["VGPRs"])
    if kernel == "k_mr_copy":
        assert int(u["LDS Size [bytes/block]"]) <= 64, u["LDS Size [bytes/block]"]


def test_item_kernel_is_what_it_is_in_the_product(usage):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"Function Name: %s\n(.*?)\n\n" % re.escape(ITEMS), r.stdout, flags=re.S)
    assert m, "k_inflate_items is missing from the product's report"
    product = {k.strip(): v.strip() for k, v in (ln.split(":", 1) for ln in m.group(1).splitlines() if ":" in ln)}
    here = usage[ITEMS]
    for f in FIELDS:
        assert here[f] == product[f], (f, here[f], product[f])
