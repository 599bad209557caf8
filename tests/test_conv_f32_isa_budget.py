"""What k_conv_f32 spends outside its MFMAs, pinned on the compiler's output: VALU issue around the K loop is taken from the MFMA pipe
(profiles/r04_mfma_valu_coissue.txt), and neither a result nor a register count shows when a set-up or a tap change grows back.
tools/conv_f32_isa_counts.py compiles tests/cpp/conv_f32_resources.hip for gfx950 with the build's flags and counts instructions per
instantiation; tests/golden/conv_f32_isa_parent.json holds the counts of the commit before the incremental tap pointers (it names it).
  1. no integer multiply (v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32, v_mad_i64_i32, v_mul_hi_i32: quarter rate or slower) between the first
     and the last MFMA of the three 16-channel-step instantiations -- the tap change adds and selects, it does not multiply (parent: 16 / 32 / 32);
  2. before the first barrier, the VALU count and the integer-multiply count are each at most half the parent's."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("sd_conv_f32_isa_counts", os.path.join(ROOT, "tools", "conv_f32_isa_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def counts(tool):
    hipcc = tool.find_hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    c = tool.counts(hipcc)
    print(tool.table(c))
    return c


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_isa_parent.json")) as f:
        g = json.load(f)
    assert len(g["commit"]) == 40
    return g["counts"]


TILES = ["16,2,2,4", "16,1,2,4", "16,1,1,4", "8,1,1,8"]


@pytest.mark.parametrize("tile", TILES[:3])
def test_no_integer_multiply_between_the_first_and_the_last_mfma(counts, parent, tile):
    assert parent[tile]["first_to_last_mfma"]["imul"] in (16, 32), "the recorded parent"
    assert counts[tile]["first_to_last_mfma"]["imul"] == 0


@pytest.mark.parametrize("tile", TILES)
def test_set_up_at_most_half_the_parents(counts, parent, tile):
    new, old = counts[tile]["before_first_barrier"], parent[tile]["before_first_barrier"]
    print(tile, "VALU %d (parent %d), integer multiplies %d (parent %d)" % (new["valu"], old["valu"], new["imul"], old["imul"]))
    assert 2 * new["valu"] <= old["valu"]
    assert 2 * new["imul"] <= old["imul"]
