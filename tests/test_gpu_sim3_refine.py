"""sd_batch_compute_sim3_refine stage by stage, each stage from the device's OWN stage input: the inlier merge against numpy, the search
against the SearchBySim3 oracle byte for byte, the built correspondences against numpy byte for byte, the optimiser against the
OptimizeSim3 oracle (bit for bit in the kernel's summation order; the chi2 decisions against the sequential oracle), then the final
matches, the gate and Scw.  Free-running scenes put ret on either side of 20, hold BoW matches that are not in KF2 (-2) and matches the
search adds that the optimiser removes."""
import numpy as np
import pytest

import fuse_cases as fc
import sim3_cases as s3
import sim3_opt_cases as so
import sim3_refine_cases as rc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SLOTS = 8


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = fc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    yield w
    w.close()


check_scene = rc.check_refine


def test_refine_stage_by_stage(ws):
    scene = rc.refine_scene(3, 300, 3, not_found=(1,))
    got, seen = check_scene(ws, scene)
    assert seen["not_run"] == 1 and min(seen["ret"]) >= 20 and seen["added"] > 20 and seen["minus2"] > 0


def test_refine_ret_on_either_side_of_the_gate(ws):
    rets = []
    for n_points in (300, 60, 34):
        got, seen = check_scene(ws, rc.refine_scene(11, n_points, 2))
        rets += seen["ret"]
    assert any(r >= 20 for r in rets) and any(r < 20 for r in rets), rets


def test_refine_removes_a_match_the_search_added(ws):
    """Two pixels of noise on the features: SearchBySim3 still pairs them inside its window, and the optimiser's chi2 check removes the
    worst of what it added (at octave 0 an error above 3.2 px exceeds th2 = 10)."""
    total = 0
    for seed in (21, 22):
        scene = rc.refine_scene(seed, 300, 2, prior_noise=0.004, noise=2.0)
        got, seen = check_scene(ws, scene, fix_scale=bool(seed & 1))
        total += seen["added_then_removed"]
    assert total > 10


def test_refine_tables_grow_with_a_larger_second_call(gpu, fe, synth):
    """A fresh workspace: one job, then three (the search's tables and the refine tables grow in one call), then the first call again."""
    w = fc.Workspace(fe, 6, tc.vocabulary(synth, 5))
    try:
        small, big = rc.refine_scene(31, 120, 1), rc.refine_scene(32, 120, 3)
        for scene in (small, big, small):
            check_scene(w, scene)
    finally:
        w.close()


def test_refine_job_independence_and_refusals(ws, fe):
    scene = rc.refine_scene(5, 200, 4, not_found=(2,))
    got, _ = check_scene(ws, scene)
    alone = dict(scene, pairs=scene["pairs"][3:4])
    one = rc.device_refine(ws, alone, upload=False)[0]
    assert one["result"].tobytes() == got[3]["result"].tobytes() and np.array_equal(one["final12"], got[3]["final12"])
    with pytest.raises(fe.SdError) as e:
        ws.b.download_sim3_refine(1)
    assert e.value.code == fe.SD_ERR_INVALID
    bad = dict(scene, pairs=[dict(scene["pairs"][0], p1=np.where(np.arange(len(scene["pairs"][0]["p1"])) == 0, len(scene["points"]) + 5, scene["pairs"][0]["p1"]))])
    with pytest.raises(fe.SdError) as e:                        # a point index outside the table: refused, not answered
        rc.device_refine(ws, bad, upload=False)
    assert e.value.code == fe.SD_ERR_INVALID
