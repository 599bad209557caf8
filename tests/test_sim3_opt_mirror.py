"""host/Optimizer.h's ORB_SLAM2::Optimizer::OptimizeSim3 (over sd_sim3_optimize_host): the header compiles with g++ against minimal
key-frame and map-point types and links against the library; on the GPU the program optimises one clean pair."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(fe, tmp_path):
    exe = str(tmp_path / "sim3_opt_mirror")
    lib_dir = os.path.dirname(fe.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "slam-dynamic_amd", "host"),
                           os.path.join(ROOT, "tests/cpp/sim3_opt_mirror_main.cpp"), "-o", exe, "-L" + lib_dir, "-lsd_frontend",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_the_mirror_compiles_and_links(fe, tmp_path):
    assert os.path.exists(build(fe, tmp_path))


@pytest.mark.gpu
def test_the_mirror_optimises_a_clean_pair(gpu, fe, tmp_path):
    out = subprocess.run([build(fe, tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "OptimizeSim3 = 39" in out.stdout, out.stdout + out.stderr
