"""The scalar staging walk's address arithmetic on the host: tests/cpp/conv_f32_offsets_check.cpp (g++ alone; what it checks per request, lane,
tap and step is written at its top) over every convolution the two unconditional k_conv_f32 tiles run
  - of YOLOv3 at the headline's 640 x 480 and at 352 x 224 (odd maps: 11 x 7 under a stride-2 layer) for batches 1, 2, 3, 128 and 256 -- at 256 the
    first layers' tensors lie beyond 4 GiB and the anchors must be exact in 64 bits;
  - of the crafted lists of tests/yolo_cases.py at their own sizes and batches (1 x 1 ... 5 x 3 maps, tiles that span many images)."""
import os
import subprocess

import pytest

import yolo_cases as yc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = (1, 2, 3, 128, 256)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_f32_offsets")
    out = str(d / "conv_f32_offsets_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "slam-dynamic_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpp", "conv_f32_offsets_check.cpp")])
    return out, d


def _run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("net", [(640, 480), (352, 224)], ids=lambda s: "%dx%d" % s)
def test_yolov3_every_tile_chunk_tap_and_step(exe, net):
    lines = _run(exe[0], [v for n in BATCHES for v in (net[0], net[1], n)])
    assert len(lines) == len(BATCHES) and all(l.endswith(": ok") and " 73 layers" in l for l in lines)


def test_the_crafted_lists(exe):
    args, want = [], 0
    for k, c in enumerate(yc.CASES):
        path = str(exe[1] / ("list_%d.txt" % k))
        with open(path, "w") as f:
            for l in c.layers:
                f.write(" ".join(str(int(v)) for v in (l["type"], l["filters"], l["size"], l["stride"], l["batch_normalize"], l["leaky"], l["from"][0], l["from"][1],
                                                       l["nfrom"], l["mask"][0], l["mask"][1], l["mask"][2])) + "\n")
        args += ["--layers", path]
        for b in c.batches:
            args += [c.net_w, c.net_h, b]
            want += 1
    lines = _run(exe[0], args)
    assert len(lines) == want and all(l.endswith(": ok") for l in lines)
    assert sum(int(l.split(":")[1].split()[0]) for l in lines) >= 30, "the lists reach the two tiles"
