"""The CPU oracle of the relocalisation matcher (tests/cpp/reloc_oracle.cpp) on the crafted scenes of reloc_cases.py: every rule of
ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) is witnessed by its branch counter, every deliberately
wrong twin fails at least one case, a numpy restatement agrees on every scene, and the 1-ulp scans record what -ffp-contract=fast
would change."""
import numpy as np
import pytest

import reloc_cases as rc
import triangulate_cases as tc


@pytest.fixture(scope="module")
def crafted():
    sc = rc.crafted_scene()
    return sc, rc.cpu_search(sc)


def test_every_rule_has_a_crafted_case(crafted):
    sc, (res, br) = crafted
    rc.check_expect(sc, res)
    for name in ("null", "bad", "found", "out_u", "out_v", "dist_min", "dist_max", "window_empty", "no_free", "above_dist", "matched", "culled",
                 "z_negative_searched", "u_eq_minx", "u_eq_maxx", "v_eq_maxy", "dist_eq_min", "dist_eq_max", "level_0", "level_top", "octave_below",
                 "octave_above", "octave_lm1", "octave_l", "octave_lp1", "clip_left", "clip_right", "clip_bottom", "on_radius", "held_on_entry",
                 "taken_by_earlier", "loser_second_choice", "tie_first_wins", "dist_eq_orb", "dist_orb_plus_1", "dist_256", "bin_wrap",
                 "culled_had_blocked"):
        assert br[name] > 0, "no crafted case takes the branch " + name
    fp, frm, ex, best, nm = res[0]
    assert nm == int((frm >= 0).sum()) == int((ex == rc.X["matched"]).sum())
    # a culled feature leaves no trace in the result rows, a matched one carries its keyframe feature's point
    job = sc["jobs"][0]
    for f in np.nonzero(frm >= 0)[0]:
        assert fp[f] == job["kf_point"][frm[f]]


def test_v_on_the_lower_image_bound():
    sc = rc.v_min_scene()
    res, br = rc.cpu_search(sc, cam=rc.CAM_VMIN)
    rc.check_expect(sc, res)
    assert br["v_eq_miny"] == 1 and br["out_v"] == 1 and br["clip_top"] >= 1
    rc.assert_same(sc, rc.numpy_search(sc, cam=rc.CAM_VMIN), res, "numpy")


def test_nan_and_infinite_projections():
    sc = rc.nan_scene()
    res, br = rc.cpu_search(sc)
    rc.check_expect(sc, res)
    assert br["nan_projection"] == 1 and br["out_u"] == 1


@pytest.mark.parametrize("twin", [t for t in rc.TWINS if t != "none"])
def test_every_wrong_twin_fails_a_case(crafted, twin):
    sc, (res, _) = crafted
    wrong, _ = rc.cpu_search(sc, twin=twin)
    with pytest.raises(AssertionError):
        rc.assert_same(sc, wrong, res, twin)
    with pytest.raises(AssertionError):
        rc.check_expect(sc, wrong)


def _scenes():
    yield rc.crafted_scene()
    yield rc.nan_scene()
    for n, nf in ((0, None), (1, None), (63, None), (64, None), (65, None), (129, None), (5, 0)):
        yield rc.sized_scene(n, nf)
    yield rc.dense_window_scene(64, 66)
    yield rc.dense_window_scene(70, 64)
    yield rc.dense_window_scene(70, 66)
    yield rc.chain_scene()
    for seed in range(8):
        yield rc.random_scene(seed)


def test_numpy_restatement_agrees_on_every_scene():
    total = 0
    for sc in _scenes():
        res, _ = rc.cpu_search(sc)
        rc.assert_same(sc, rc.numpy_search(sc), res, "numpy")
        total += sum(r[4] for r in res)
    assert total > 1000


def test_random_scenes_take_every_exit():
    seen = np.zeros(len(rc.EXITS), np.int64)
    br_all = {}
    for seed in range(8):
        res, br = rc.cpu_search(rc.random_scene(seed))
        for r in res:
            seen += np.bincount(r[2], minlength=len(rc.EXITS))
        for k, v in br.items():
            br_all[k] = br_all.get(k, 0) + v
    assert np.all(seen[1:] > 0), "exits never taken: %r" % [rc.EXITS[i] for i in np.nonzero(seen[1:] == 0)[0] + 1]
    for name in ("taken_by_earlier", "held_on_entry", "loser_second_choice", "z_negative_searched", "culled"):
        assert br_all[name] > 0, name


def test_dense_window_and_chain():
    """The shapes the device's bounded key list and chunked replay turn on, as the sequential loop answers them."""
    (fp, frm, ex, best, nm), = rc.cpu_search(rc.dense_window_scene(70, 66))[0]
    assert nm == 66 and int((ex == rc.X["matched"]).sum()) == 66              # the 65th and 66th takers need keys 65 and 66 of 70
    res, br = rc.cpu_search(rc.dense_window_scene(64, 66))
    assert res[0][4] == 64 and list(res[0][2][64:]) == [rc.X["no_free"]] * 2
    sc = rc.chain_scene()
    (fp, frm, ex, best, nm), = rc.cpu_search(sc)[0]
    assert nm == 65 and list(frm[:65]) == sc["want_chain"] and frm[65] == -1
    assert list(best[1:, 1]) == [60] * 64                                     # every one but the first took its second choice


@pytest.mark.parametrize("kind", rc.SCAN_KINDS)
def test_threshold_scans(kind):
    sc = rc.scan_scene(kind)
    reached = rc.scan_reached(sc)
    per = rc.SCAN_STEPS // rc.SCAN_VARIANTS
    r = reached.reshape(rc.SCAN_VARIANTS, per)
    assert np.all(r.any(1) & ~r.all(1)), "every geometry crosses its bound inside the scan"
    assert np.all(np.abs(np.diff(r.astype(int), axis=1)).sum(1) == 1), "one crossing per geometry"
    res, _ = rc.cpu_search(sc, cam=sc["cam"])
    rc.assert_same(sc, rc.numpy_search(sc, cam=sc["cam"]), res, "numpy")
    if tc.host_has_fma():
        changed = int((rc.scan_reached(sc, "fast") != reached).sum())
        print("scan %s: %d of %d decisions change under -ffp-contract=fast" % (kind, changed, rc.SCAN_STEPS))


# ---------------------------------------------------------------- the cascade (Tracking.cc:2292-2358)
@pytest.fixture(scope="module")
def cascade():
    sc = rc.cascade_scene()
    return sc, rc.cpu_refine(sc)


def test_cascade_cases_sit_on_every_gate(cascade):
    """nGood 9 / 10 at :2313, 49 / 50 at :2321, the sum 49 / 50 at :2325, nGood 30 / 31 and 49 / 50 at :2331, the sum 49 / 50 at :2340,
    nGood 49 / 50 at :2354."""
    sc, res = cascade
    for name, want, r in zip(sc["names"], sc["want"], res):
        assert rc.decisions(r)[:4] == want, "%s: %r, meant %r" % (name, rc.decisions(r)[:4], want)
    by = dict(zip(sc["names"], res))
    # no outlier is set to NULL after the second optimisation: they are in the final assignment, flagged
    r, fp, o = by["2331_ngood_30"]
    assert int(((fp >= 0) & (o == 1)).sum()) == 20
    # ... and after the third they are gone; a key point whose outlier was set to NULL keeps its flag
    r, fp, o = by["2354_ngood_49"]
    assert int(((fp >= 0) & (o == 1)).sum()) == 0 and int(((fp < 0) & (o == 1)).sum()) == 2 + 5 + 1
    for r, fp, o in res:
        assert r["Tcw"].tobytes() == r["Tcw_stage"][2].tobytes()


@pytest.mark.parametrize("twin,case", [("discard_after_second_optimisation", "2331_ngood_30"), ("ge_30", "2331_ngood_30")])
def test_every_wrong_cascade_twin_fails_a_case(cascade, twin, case):
    sc, res = cascade
    q = sc["names"].index(case)
    wrong = rc.cpu_refine(sc, twin=twin)
    assert rc.decisions(wrong[q]) != rc.decisions(res[q])


def test_cascade_decisions_do_not_hang_on_the_pose(cascade):
    """Each stage pose perturbed by what pose_close tolerates (1e-5, the bar test_gpu_pose.py holds the device to): every decision, the
    final assignment and the outlier flags stay."""
    sc, res = cascade
    rng = np.random.default_rng(7)
    for trial in range(6):
        pert = np.array([rc.pose_perturbation(rng, j["Tcw"]) for j in sc["jobs"]])
        got = rc.cpu_refine(sc, perturb=pert)
        for name, a, b in zip(sc["names"], got, res):
            assert rc.decisions(a) == rc.decisions(b), "%s: trial %d changes a decision" % (name, trial)


def test_random_cascades_rarely_hang_on_the_pose():
    """The generator of tools/fuzz_reloc.py: fewer than 5 % of its draws change a decision under the pose tolerance, and the draws reach
    every stage."""
    rng = np.random.default_rng(11)
    n = flips = 0
    stages = set()
    for seed in range(16):
        sc = rc.random_cascade_scene(seed)
        res = rc.cpu_refine(sc)
        pert = np.array([rc.pose_perturbation(rng, j["Tcw"]) for j in sc["jobs"]])
        got = rc.cpu_refine(sc, perturb=pert)
        for a, b in zip(got, res):
            n += 1; flips += rc.decisions(a) != rc.decisions(b); stages.add(int(b[0]["stage_reached"]))
    print("random cascades: %d of %d draws change a decision under the pose tolerance; stages reached %r" % (flips, n, sorted(stages)))
    assert flips * 20 <= n and {1, 2, 3}.issubset(stages)
