"""Register budget of k_conv_f32 (csrc/k_yolo32.h): the 128-filter tile runs three workgroups per CU on 166 of the 170 VGPRs that three
waves per SIMD leave it, the 64-filter tile on 168; a few registers more in an epilogue or prologue cost a wave per SIMD or spill into
scratch without any test of results noticing.  Compiles tests/cpp/conv_f32_resources.hip (the four instantiations the detector launches)
for gfx950 with the build's own flags and asserts, per kernel: no scratch, no spills, occupancy not below what the parent of the epilogue
change had (3 / 3 / 3 / 4 waves per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as graft

HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
MIN_OCCUPANCY = {(16, 2, 2, 4): 3, (16, 1, 2, 4): 3, (16, 1, 1, 4): 3, (8, 1, 1, 8): 4}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not HIPCC:
        pytest.skip("hipcc not found")
    flags = [f for f in graft.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path_factory.mktemp("conv_f32_resources") / "conv_f32_resources.o"
    r = subprocess.run([HIPCC] + flags + ["-I" + graft.CSRC, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(out),
                                          os.path.join(graft.ROOT, "tests", "cpp", "conv_f32_resources.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    table, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        f = re.match(r"Function Name: _Z10k_conv_f32ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEv", text)
        if f:
            cur = table.setdefault(tuple(int(v) for v in f.groups()), {})
        elif text.startswith("Function Name:"):
            cur = None
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            if v.strip().isdigit():
                cur[k.strip()] = int(v)
    return table


@pytest.mark.parametrize("tile", sorted(MIN_OCCUPANCY))
def test_no_scratch_no_spills_and_the_parents_occupancy(usage, tile):
    assert tile in usage, "no resource remarks for k_conv_f32<%d, %d, %d, %d>" % tile
    u = usage[tile]
    print(tile, u)
    assert u["ScratchSize [bytes/lane]"] == 0
    assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0
    assert u["Occupancy [waves/SIMD]"] >= MIN_OCCUPANCY[tile]
