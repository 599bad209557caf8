"""The LocalBundleAdjustment CPU oracle (tests/cpp/ba_oracle.cpp) on the crafted scenes of ba_cases.py: every case reaches the branch it
is named for, the solver does what a bundle adjustment must, every decision of every case stays clear of its threshold, and the
yardstick for the device tolerance (DESIGN Q37) is measured and recorded."""
import json
import os

import numpy as np
import pytest

import ba_cases as bc

TOLERANCE_JSON = os.path.join(bc.ROOT, "profiles", "ba_tolerance.json")


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_reaches_its_branches(name):
    r = bc.expected(name)
    for b in bc.CASES[name][1]:
        assert r["branches"][b] > 0, "%s never reached %s: %r" % (name, b, r["branches"])
    assert r["branches"]["factor_fail"] == 0


def test_structure_of_the_named_cases():
    assert bc.expected("small")["branches"]["pose_pose"] == 0
    assert len(bc.scene("small")["kfs"]) == 3 and len(bc.scene("small")["xw"]) == 8
    assert bc.expected("far_start")["stats"]["rejected"].sum() >= 1
    st = bc.expected("at_optimum")["stats"]
    assert st["iterations"][0] < 5 or st["iterations"][1] < 10          # the three-in-a-row stop cut a round short
    for name in ("empty_no_edges", "empty_no_points", "empty_nothing"):
        s, r = bc.scene(name), bc.expected(name)
        assert r["stats"]["iterations"].tolist() == [0, 0] and r["stats"]["trials"].tolist() == [0, 0]
        assert np.array_equal(r["Tcw"].reshape(-1, 16), s["kfs"]["Tcw"][:s["n_local"]]) and np.array_equal(r["xw"], s["xw"])
    for n, name in ((bc.THREADS - 1, "edges_m1"), (bc.THREADS, "edges_0"), (bc.THREADS + 1, "edges_p1")):
        assert len(bc.scene(name)["edges"]) == n
    for d, name in ((-6, "tile_m6"), (0, "tile_0"), (6, "tile_p6")):
        assert 6 * bc.scene(name)["n_local"] == bc.CHOL_TILE + d


def test_inactive_vertices_keep_their_estimate():
    # the point all of whose edges went to level 1 is not in round 2's index mapping: it comes out with the value round 1 left it with
    # (the oracle's test hook hands that out), while the points round 2 works on move
    s, r = bc.scene("point_all_level1"), bc.run_oracle(bc.problem_of(bc.scene("point_all_level1")))
    idx = np.flatnonzero(s["edges"]["point"] == 5)
    assert r["level1"][idx].all() and r["erase"][idx].all()
    assert r["branches"]["point_inactive"] >= 1
    assert np.array_equal(r["xw"][5], r["round1_xw"][5].astype(np.float32))
    moved = np.abs(r["xw"].astype(np.float64) - r["round1_xw"]).max(1) > 1e-4
    assert not moved[5] and moved.sum() >= len(moved) // 2
    s, r = bc.scene("kf_all_level1"), bc.expected("kf_all_level1")
    assert r["level1"][s["edges"]["kf"] == 2].all()
    assert r["branches"]["kf_inactive"] >= 1


def test_duplicate_edges_add_up():
    # two edges on one (keyframe, point) pair weigh like one edge of the summed information at the mean observation, to first order:
    # the adjustment stays close to the scene without the duplicates and every decision is taken
    s, r = bc.scene("duplicate_edge"), bc.expected("duplicate_edge")
    assert r["branches"]["duplicate_edge"] >= 2                # a local-keyframe pair meets its block again (a fixed one has no block)
    n = len(s["edges"]) - 3
    base = bc.run_oracle(dict(bc.problem_of(s), edges=s["edges"][:n]))
    assert np.array_equal(r["erase"][:n], base["erase"]) and not r["erase"][n:].any()
    assert np.abs(r["xw"] - base["xw"]).max() < 0.05 and np.abs(r["Tcw"] - base["Tcw"]).max() < 5e-3


def test_noise_free_scene_returns_the_ground_truth():
    s, r = bc.scene("noise_free"), bc.expected("noise_free")
    assert np.abs(r["Tcw"] - s["gt_T"][:s["n_local"]]).max() < 2e-4          # f32 observations: ~1e-5 px
    assert np.abs(r["xw"] - s["gt_xw"]).max() < 2e-3
    assert r["stats"]["n_erased"] == 0 and r["stats"]["chi2"][1] < 1e-3


def test_planted_outliers_are_erased_and_nothing_else():
    s, r = bc.scene("outliers"), bc.expected("outliers")
    assert np.array_equal(np.flatnonzero(r["erase"]), s["planted"])
    assert np.array_equal(np.flatnonzero(r["level1"]), s["planted"])
    assert r["stats"]["n_erased"] == len(s["planted"]) == r["stats"]["n_level1"]


def test_normal_and_distance():
    s, r = bc.scene("mixed"), bc.expected("mixed")
    T = np.array(s["kfs"]["Tcw"]).reshape(-1, 4, 4).astype(np.float64)
    T[:s["n_local"]] = r["Tcw"]
    Ow = np.stack([-t[:3, :3].T @ t[:3, 3] for t in T])
    for p in range(len(s["xw"])):
        e = s["edges"][(s["edges"]["point"] == p) & (r["erase"] == 0)]
        d = r["xw"][p].astype(np.float64) - Ow[e["kf"]]
        n = (d / np.linalg.norm(d, axis=1)[:, None]).mean(0)
        assert np.abs(n - r["normal"][p]).max() < 1e-6
        k = s["ref_kf"][p]
        assert r["dist"][p] == -1 if k < 0 else abs(r["dist"][p] - np.linalg.norm(r["xw"][p] - Ow[k])) < 1e-5


@pytest.mark.parametrize("name", list(bc.CASES))
def test_every_decision_is_outside_the_margin(name):
    r = bc.expected(name)
    for k, v in r["margins"].items():
        assert v >= bc.MARGIN, "%s: a %s decision at relative distance %.3g from its threshold" % (name, k, v)


def spread(name):
    sp = bc.spread_of(bc.problem_of(bc.scene(name)), bc.expected(name))
    assert sp is not None, "%s: a variant of the oracle takes another decision" % name
    return sp


def test_tolerance_yardstick_is_recorded():
    rec = {name: spread(name) for name in bc.CASES}
    for name, sp in rec.items():           # an ill-conditioned case would show here: a spread beyond a few f32 ulps of metre-sized entries
        assert max(sp.values()) < 2e-5, (name, sp)
    text = json.dumps(dict(what="largest |difference| of the oracle's f32 outputs between the build with -ffp-contract=off and (a) "
                                "-ffp-contract=fast, (b) the edges in reversed insertion order; per crafted case of tests/ba_cases.py",
                           cases=rec), indent=1, sort_keys=True) + "\n"
    old = open(TOLERANCE_JSON).read() if os.path.exists(TOLERANCE_JSON) else None
    if old != text:
        with open(TOLERANCE_JSON, "w") as f:
            f.write(text)
