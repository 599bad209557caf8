"""The refine chain's scenes (tests/sim3_refine_cases.py) free-running on the CPU -- numpy stages, the SearchBySim3 oracle, the OptimizeSim3
oracle -- without a GPU: the scenes reach what test_gpu_sim3_refine.py needs them for."""
import sim3_refine_cases as rc
import triangulate_cases as tc


def test_scenes_reach_the_gate_the_skip_and_a_removed_addition():
    lv = tc.Levels()
    rets = [j["ret"] for n in (300, 60, 34) for j in rc.cpu_refine(rc.refine_scene(11, n, 2), lv, 4096)]
    assert 19 in rets and 22 in rets and max(rets) > 90           # ret on either side of the gate, one step away from it
    jobs = rc.cpu_refine(rc.refine_scene(3, 300, 3, not_found=(1,)), lv, 4096)
    assert [j["ran"] for j in jobs] == [1, 0, 1] and all(j["minus2"] > 0 and j["added"] > 20 for j in jobs if j["ran"])
    noisy = [j for seed in (21, 22) for j in rc.cpu_refine(rc.refine_scene(seed, 300, 2, prior_noise=0.004, noise=2.0), lv, 4096, fix_scale=bool(seed & 1))]
    assert sum(j["added_then_removed"] for j in noisy) > 10 and all(j["ret"] >= 20 for j in noisy)
