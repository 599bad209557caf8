"""The staging addresses of k_conv_f32's two unconditional tiles walk in scalar registers (k_yolo32.h, "The scalar walk"), pinned on the
compiler's output.  tools/conv_f32_loop_gaps.py compiles tests/cpp/conv_f32_resources.hip for gfx950 with the build's flags and splits every K
step in the text into the gaps between consecutive v_mfma; tests/golden/conv_f32_walk_parent.json holds the per-step counts of the commit before
the change (it names it; printed once from that commit's tree with the tool's --json, never regenerated from the code under test).

For <16, 2, 2, 4> and <16, 1, 2, 4>, on the two steps of the loop (a "whole loop step" is the text from the step's first MFMA to the barrier
behind it, tap-change block included: the tool's loop_part):
  1. between a step's first and last MFMA no VALU instruction writes a register a staging load takes its address from; on the placed tile
     (<16, 2, 2, 4>) a load's gap holds the load alone among vector instructions: no VALU, no LDS and no second vector-memory instruction
     (scalar adds and compares issue in the scalar pipe and stand where the scheduler puts them);
  2. the VALU count of a whole loop step is at most half the parent's;
  3. every vector-memory instruction of the steps is a buffer_load_dwordx4;
  4. no s_and_saveexec and no v_readfirstlane stands within the steps: the descriptors are uniform to the compiler, no waterfall loop.
The two 32-filter tiles keep their pointers and their conditional request:
  5. their steps' instruction counts by class are the parent's."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK = [(16, 2, 2, 4), (16, 1, 2, 4)]
PLACED = [(16, 2, 2, 4)]
KEPT = [(16, 1, 1, 4), (8, 1, 1, 8)]


def _tool():
    spec = importlib.util.spec_from_file_location("sd_conv_f32_loop_gaps", os.path.join(ROOT, "tools", "conv_f32_loop_gaps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _key(tile):
    return ",".join(str(v) for v in tile)


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def text(tool):
    hipcc = tool.TOOL.find_hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    t = tool.TOOL.assembly(hipcc)
    print(tool.report(t))
    return t


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_walk_parent.json")) as f:
        g = json.load(f)
    assert len(g["commit"]) == 40
    return g["steps"]


def _steps(tool, text, tile):
    st = tool.steps(tool.body(text, tile))
    assert len(st) == 3, "two steps in the loop and one behind it"
    return st


@pytest.mark.parametrize("tile", WALK)
def test_no_valu_writes_a_staging_address_between_the_mfmas(tool, text, tile):
    for si, st in enumerate(_steps(tool, text, tile)[:2]):
        loads = tool.staging_loads(st)
        assert loads and all(reg for _, _, reg in loads), "step %d: %s" % (si, loads)
        for g, gap in enumerate(st[1:]):
            for _, _, reg in loads:
                assert not tool.valu_writes(gap, reg), "step %d, behind MFMA %d: %s" % (si, g, tool.valu_writes(gap, reg))


@pytest.mark.parametrize("tile", PLACED)
def test_a_loads_gap_holds_the_load_alone(tool, text, tile):
    for si, st in enumerate(_steps(tool, text, tile)[:2]):
        seen = 0
        for g, gap in enumerate(st[1:]):
            c = tool.gap_counts(gap)
            if c["vmem"]:
                seen += c["vmem"]
                assert (c["vmem"], c["valu"], c["ds_read"], c["ds_write"]) == (1, 0, 0, 0), "step %d, behind MFMA %d: %s" % (si, g, c)
        assert seen == 4, "step %d: the stage's four loads stand between the MFMAs" % si


@pytest.mark.parametrize("tile", WALK)
def test_valu_of_a_loop_step_at_most_half_the_parents(tool, text, parent, tile):
    for si, st in enumerate(_steps(tool, text, tile)[:2]):
        new, old = tool.gap_counts(tool.loop_part(st))["valu"], parent[_key(tile)][si]["loop"]["valu"]
        print(tile, "step %d: VALU %d (parent %d)" % (si, new, old))
        assert old >= 20, "the recorded parent"
        assert 2 * new <= old


@pytest.mark.parametrize("tile", WALK)
def test_every_staging_load_is_a_buffer_load(tool, text, tile):
    st = _steps(tool, text, tile)
    for si, s in enumerate(st):
        ops = [op for op, _, _ in tool.staging_loads(s)] + [op for op, _ in (s[0] if si else []) if tool.classify(op) == "vmem"]
        assert all(op == "buffer_load_dwordx4" for op in ops), "step %d: %s" % (si, ops)
    assert sum(len(tool.staging_loads(s)) for s in st[:2]) == 2 * (5 if tile == (16, 1, 2, 4) else 4)


@pytest.mark.parametrize("tile", WALK)
def test_no_waterfall_loop_within_the_steps(tool, text, tile):
    for si, s in enumerate(_steps(tool, text, tile)):
        part = tool.loop_part(s) + (list(s[0]) if si else [])
        bad = [op for op, _ in part if op.startswith(("s_and_saveexec", "v_readfirstlane"))]
        assert not bad, "step %d: %s" % (si, bad)


@pytest.mark.parametrize("tile", KEPT)
def test_the_32_filter_tiles_steps_are_the_parents(tool, text, parent, tile):
    new = tool.step_counts(text)[_key(tile)]
    assert new == parent[_key(tile)]
