"""k_conv_f32 divides by multiply-high with numbers made on the host (sd_magic_div / yolo_f32_setup, csrc/sd_yolo_plan.h): pixel -> (image, row,
column) and workgroup -> (filter-tile group, pixel tile, filter tile).  A wrong quotient would send a workgroup or a gather to another pixel
without any error, so the host code is checked here, on the CPU, against plain division over the FULL ranges of every convolution of
yolov3.cfg at 640 x 480 and batch 1, 3, 128 and 256 (tests/cpp/conv_f32_magic_check.cpp, compiled with g++ alone), at the small network
sizes of the GPU tests, and at the ends of the range the formula is stated for."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(640, 480, 1), (640, 480, 3), (640, 480, 128), (640, 480, 256), (160, 96, 3), (96, 64, 3), (64, 32, 5), (32, 32, 1)]


@pytest.fixture(scope="module")
def report():
    d = tempfile.mkdtemp(prefix="conv_f32_magic_")
    exe = os.path.join(d, "conv_f32_magic_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "slam-dynamic_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "conv_f32_magic_check.cpp")])
    r = subprocess.run([exe] + [str(v) for c in CASES for v in c], capture_output=True, text=True)
    out = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(edges|case (\d+) (\d+) (\d+)): (\d+) checked, (\d+) wrong", line)
        assert m, line
        key = "edges" if m.group(1) == "edges" else tuple(int(m.group(i)) for i in (2, 3, 4))
        out[key] = (int(m.group(5)), int(m.group(6)))
    assert r.returncode in (0, 2), r.stderr
    return out


def test_edges_of_the_range(report):
    checked, wrong = report["edges"]
    assert checked > 1000 and wrong == 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d n=%d" % c)
def test_every_division_of_every_layer_over_its_full_range(report, case):
    checked, wrong = report[case]
    w, h, n = case
    assert checked > n * w * h, "at least the first layer's pixels"      # layer 0 alone divides n w h pixel indices
    assert wrong == 0
