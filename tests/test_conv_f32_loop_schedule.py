"""The shape of k_conv_f32's K step in the compiler's output, pinned: neither a result nor a register count shows when the step's staging
collapses back into one clump or its waits stop being counted.  tools/conv_f32_loop_gaps.py compiles tests/cpp/conv_f32_resources.hip for
gfx950 with the build's flags and splits every K step in the text into the gaps between consecutive v_mfma.

The two instantiations whose weight rows fill their threads (<16, 2, 2, 4>, <16, 1, 2, 4>) request every stage unconditionally and have a
straight-line step; the 128-filter tile <16, 2, 2, 4> (69 of the detector's 75 layers) has its staging placed (k_yolo32.h, sd_f32_place).  The
two 32-filter tiles keep the conditional request inside the step (measured slower without it) and are held to 4 alone.
  1. straight-line: no s_cbranch between a step's first and last v_mfma (the loop's back edge and the tap change stand behind the last one).
  2. placed: no gap between two consecutive v_mfma holds more than one vector-memory instruction, more than two LDS instructions or more than
     eight other VALU instructions (8 x 4 cycles of issue, half of the 56 cycles a 64-cycle MFMA leaves free behind its own 8).
  3. counted waits on the changed tile with two register sets (DEEP), the 128-filter tile: every s_waitcnt vmcnt(N) of a loop step leaves at
     least one whole stage's requests in flight, N >= 4, its loads per stage.  (Before: vmcnt(3..0): each ds_write also waited for the loads issued
     one step earlier.)
  4. occupancy: <16, 2, 2, 4> within 170 VGPRs (three workgroups per CU) and no private segment; the other tiles keep their waves per SIMD (3, 3, 5
     by registers) and have no private segment either."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRAIGHT = [(16, 2, 2, 4), (16, 1, 2, 4)]
PLACED = [(16, 2, 2, 4)]
DEEP_LOADS = {(16, 2, 2, 4): 4}      # tile: loads per stage and thread (WC + XC)
WAVES = {(16, 2, 2, 4): 3, (16, 1, 2, 4): 3, (16, 1, 1, 4): 3, (8, 1, 1, 8): 5}


def _tool():
    spec = importlib.util.spec_from_file_location("sd_conv_f32_loop_gaps", os.path.join(ROOT, "tools", "conv_f32_loop_gaps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def _steps(tool, text, tile):
    st = tool.steps(tool.body(text, tile))
    assert len(st) == 3 and len({len(s) for s in st}) == 1, "two steps in the loop and one behind it, the same MFMAs in each"
    return st


@pytest.mark.parametrize("tile", STRAIGHT)
def test_no_branch_between_the_first_and_the_last_mfma_of_a_step(tool, text, tile):
    for si, st in enumerate(_steps(tool, text, tile)):
        for g, gap in enumerate(st[1:]):
            assert not [op for op, _ in gap if tool.classify(op) == "branch"], "step %d, behind MFMA %d" % (si, g)


@pytest.mark.parametrize("tile", PLACED)
def test_no_gap_collects_the_staging(tool, text, tile):
    for si, st in enumerate(_steps(tool, text, tile)):
        total = dict.fromkeys(tool.CLASSES, 0)
        for g, gap in enumerate(st[1:]):
            c = tool.gap_counts(gap)
            for k in c:
                total[k] += c[k]
            where = "step %d, behind MFMA %d: %s" % (si, g, c)
            assert c["vmem"] <= 1 and c["ds_read"] + c["ds_write"] <= 2 and c["valu"] <= 8, where
        if si < 2:      # the loop's steps: the whole stage is written and the next one requested between the MFMAs, not behind them
            assert total["ds_write"] == 4 and total["vmem"] == 4, "step %d: %s" % (si, total)


@pytest.mark.parametrize("tile", sorted(DEEP_LOADS))
def test_waits_on_the_deep_tiles_are_counted(tool, text, tile):
    for si, st in enumerate(_steps(tool, text, tile)[:2]):
        waits = tool.vmcnt_waits(st)
        assert waits, "step %d: the stage's ds_writes wait for their loads inside the step" % si
        assert min(waits) >= DEEP_LOADS[tile], "step %d: vmcnt waits %s" % (si, waits)


@pytest.mark.parametrize("tile", sorted(WAVES))
def test_registers_and_private_segment(tool, text, tile):
    md = tool.metadata(text, tile)
    print(tile, md)
    assert md["private_segment_fixed_size"] == 0
    assert md["waves_per_simd"] == WAVES[tile]
    if tile == (16, 2, 2, 4):
        assert md["vgpr_count"] <= 170
