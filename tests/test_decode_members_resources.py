"""What the kernels of zz_decode_members_device cost a CU (CPU only: hipcc cross-compiles gfx950): none of them spills or uses
scratch, and the serial path's k_inflate_members needs no more LDS than k_inflate_serial, whose form it has. The test compiles
a translation unit of its own that holds zz_inflate_members.h and what it includes -- the decode kernels, not the encoders."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["k_members_markILb0E", "k_members_markILb1E", "k_members_scan", "k_members_check", "k_members_hop", "k_members_slots",
       "k_inflate_members"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    d = tmp_path_factory.mktemp("members_resources")
    src = d / "members.hip"
    csrc = os.path.join(ROOT, "zzflate_amd", "csrc")
    header = (os.path.join(csrc, "zz_checksum.h"), os.path.join(csrc, "zz_inflate_members.h"))      # (in zz_api.hip's order)
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s"\n#include "%s"\n'
                   "template __global__ void zz::k_members_mark<false>(const uint8_t*, uint64_t, uint32_t*, const uint64_t*, uint64_t*, uint32_t*);\n"
                   "template __global__ void zz::k_members_mark<true>(const uint8_t*, uint64_t, uint32_t*, const uint64_t*, uint64_t*, uint32_t*);\n" % header)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(d / "members.s"), str(src)], capture_output=True, text=True, timeout=900)
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
    # scalar registers parked in lanes of a vector register touch no memory; the inflate core does that in every kernel
    # that holds it (k_inflate_items among them), the other new kernels not at all
    if kernel == "k_inflate_members":
        assert int(u["SGPRs Spill"]) <= int(find(usage, "k_inflate_items")["SGPRs Spill"])
    else:
        assert int(u["SGPRs Spill"]) == 0
    assert u["Dynamic Stack"] == "False"


def test_serial_members_kernel_needs_no_more_lds_than_the_serial_kernel(usage):
    members = int(find(usage, "k_inflate_members")["LDS Size [bytes/block]"])
    serial = int(find(usage, "k_inflate_serial")["LDS Size [bytes/block]"])
    assert members <= serial, (members, serial)


def test_mark_kernel_is_light(usage):
    # a bandwidth pass: full occupancy (at most 64 VGPRs at 256 lanes a workgroup) and next to no LDS
    for k in ("k_members_markILb0E", "k_members_markILb1E"):
        u = find(usage, k)
        assert int(u["VGPRs"]) <= 64, (k, u["VGPRs"])
        assert int(u["LDS Size [bytes/block]"]) <= 64, (k, u["LDS Size [bytes/block]"])
