"""The CPU oracle of the loop-closing matchers (tests/cpp/loop_oracle.cpp) on its own: every crafted case of loop_cases.py reaches the
branch it was built for (the oracle's counters), a numpy restatement of the three functions agrees with it on every scene, and each
rule has a wrong twin that some crafted case tells apart.  The device tests (test_gpu_loop.py) compare the library with this oracle."""
import numpy as np
import pytest

import fuse_cases as fc
import loop_cases as lc
import triangulate_cases as tc


@pytest.fixture(scope="module")
def bow(synth, orc):
    O = orc.Vocabulary.from_nodes(tc.vocabulary(synth, 5))
    voc, cases = lc.bow_cases(synth, O)
    return voc, O, cases


@pytest.fixture(scope="module")
def crafted():
    return lc.crafted_scene()


@pytest.fixture(scope="module")
def projection():
    return lc.projection_scene()


def same_fuse(a, b):
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2] for x, y in zip(a, b)) and len(a) == len(b)


def same_project(a, b):
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2] for x, y in zip(a, b)) and len(a) == len(b)


# ---------------------------------------------------------------- Q41
def test_decomposition_is_the_frozen_statement():
    rng = np.random.default_rng(1)
    for q in range(200):
        T = tc.pose(tc.rodrigues(rng.normal(size=3)), rng.normal(size=3) * 3)
        S = lc.similarity(T, float(rng.uniform(0.2, 5.0)))
        assert lc.decompose(S).tobytes() == lc.decompose_numpy(S).tobytes()
    # a power-of-two scale over a pose whose first row has norm 1 in f32 gives the pose back bit for bit
    T = tc.pose(tc.rodrigues([0.3, 0.0, 0.0]), [0.1, -0.2, 0.3]).astype(np.float32)
    for s in (1.0, 0.5, 2.0):
        assert lc.decompose(lc.similarity(T, s)).tobytes() == T.tobytes()


# ---------------------------------------------------------------- Fuse(pKF, Scw, ...)
def test_crafted_fuse_cases_reach_their_branches(crafted):
    sc = lc.with_scale(crafted, 1.0)
    res, br = lc.cpu_fuse(sc)
    lc.check_crafted(sc, res)
    for name in ("entry_skip", "z_negative", "z_zero", "out_of_image", "u_eq_maxx", "u_eq_minx", "v_eq_maxy", "dist_below_min", "dist_above_max",
                 "view_angle", "window_empty", "clip_left", "clip_right", "clip_top", "clip_bottom", "octave_below", "octave_above", "octave_lm1", "octave_l",
                 "tie_earlier_wins", "dist50", "dist51", "no_features", "empty_job", "window_over_64", "fuse_dist256", "meet_kf", "meet_bad", "add",
                 "meet_candidate", "chi2_would_reject"):
        assert br[name] > 0, name
    assert br["chi2_would_reject"] >= len(lc.CHI2_ONLY)
    hits = res[0][1]
    assert set(np.unique(hits["action"])) == {fc.ADD, fc.MEET_KF, fc.MEET_BAD, fc.MEET_CANDIDATE}


def test_v_on_the_lower_image_bound():
    """A camera with cy = fy / 4 lets an f32 ordinate project onto mnMinY exactly: inside through both functions, the next float outside."""
    sc = lc.v_min_scene()
    res, br = lc.cpu_fuse(sc, cam=lc.CAM_VMIN)
    assert br["v_eq_miny"] == 1 and br["out_of_image"] == 1
    for name, (job, pos, idx, dist) in sc["expect_scw"].items():
        assert tuple(int(x) for x in res[job][0][pos]) == (idx, dist), name
    assert same_fuse(lc.numpy_fuse(sc, cam=lc.CAM_VMIN), res)
    pr, br = lc.cpu_project(sc, cam=lc.CAM_VMIN)
    assert br["v_eq_miny"] == 1 and br["out_of_image"] == 1 and pr[0][2] == 1 and pr[0][1].tobytes() == res[0][0].tobytes()
    assert same_project(lc.numpy_project(sc, cam=lc.CAM_VMIN), pr)


def test_window_of_16_and_17_columns():
    for cols, over in ((16, 0), (17, 1)):
        sc = lc.with_scale(lc.wide_window_scene(cols), 1.0)
        res, br = lc.cpu_fuse(sc)
        assert br["window_over_16_cols"] == over and tuple(res[0][0][0]) == (39, 9)
        assert same_fuse(lc.numpy_fuse(sc), res)
        pr, br = lc.cpu_project(sc)
        assert br["window_over_16_cols"] == over and pr[0][2] == 1 and same_project(lc.numpy_project(sc), pr)


@pytest.mark.parametrize("scale", lc.SCALES)
def test_scales(crafted, scale):
    """A power-of-two scale divides out exactly (Scw = s * T in f32, scw = s * n, inv = (1 / s) * fl(1 / n)): scales 0.5 and 2 give the
    bytes of scale 1 on every job, the exact image bounds of keyframe I included.  1.37 rounds, so only the anchors that do not sit on
    a float bound (keyframe A) keep their outcome.  The numpy restatement follows the oracle at every scale."""
    sc = lc.with_scale(crafted, scale)
    res, _ = lc.cpu_fuse(sc)
    assert same_fuse(lc.numpy_fuse(sc), res)
    one, _ = lc.cpu_fuse(lc.with_scale(crafted, 1.0))
    if scale in (0.5, 2.0):
        assert same_fuse(res, one)
    assert same_fuse([res[0], res[4]], [one[0], one[4]])


def test_scale_one_equals_the_plain_fuse_where_every_feature_passes_chi_square():
    """A rigid pose whose first row is (1, 0, 0) and scale 1: the decomposition returns the pose, and on a scene whose features lie on
    their projections (every one passes the chi-square test of Fuse(pKF, vpMapPoints, th)) the two searches give the same bytes."""
    sc = lc.rigid_exact_scene()
    assert lc.decompose(sc["scw"][0]).tobytes() == np.asarray(sc["kfs"][0]["Tcw"], np.float32).tobytes()
    res, br = lc.cpu_fuse(sc)
    plain, pbr = fc.cpu_run(sc)
    assert pbr["stereo_fail"] == 0 and pbr["mono_fail"] == 0 and br["chi2_would_reject"] == 0
    assert same_fuse(res, plain) and res[0][2] > 50


# ---------------------------------------------------------------- SearchByProjection(pKF, Scw, ...)
def test_crafted_projection_cases_reach_their_branches(projection):
    res, br = lc.cpu_project(projection)
    lc.check_projection(projection, res)
    for name in ("already_found", "target_matched", "taken_by_earlier", "loser_second_choice", "loser_above_th", "loser_nothing_left", "entry_skip"):
        assert br[name] > 0, name
    assert br["target_matched"] >= 2
    assert same_project(lc.numpy_project(projection), res)


def test_projection_on_the_shared_search_cases(crafted):
    for scale in lc.SCALES:
        sc = lc.with_scale(crafted, scale)
        sc["matched"] = lc.matched_from_state(sc)
        sc["th_proj"] = 3
        res, br = lc.cpu_project(sc)
        assert same_project(lc.numpy_project(sc), res)
        assert br["target_matched"] > 0 and br["dist50"] > 0 and br["dist51"] > 0 and sum(r[2] for r in res) > 10


# ---------------------------------------------------------------- SearchByBoW(pKF1, pKF2, ...)
def test_crafted_bow_cases_reach_their_branches(bow):
    _, _, cases = bow
    total = {}
    for name, c in cases.items():
        m, nm, br = lc.cpu_bow(c)
        assert nm == int((m >= 0).sum())
        for a, b in c["expect"].items():
            assert int(m[a]) == b, "%s: feature %d matched %d, meant %d" % (name, a, m[a], b)
        m2, nm2 = lc.numpy_bow(c)
        assert m.tobytes() == m2.tobytes() and nm == nm2, name
        for k, v in br.items():
            total[k] = total.get(k, 0) + v
    for k in lc.BRANCHES:
        if k.startswith("bow_"):
            assert total[k] > 0, k
    assert lc.cpu_bow(cases["rotation"])[1] == lc.cpu_bow(cases["rotation_off"])[1] - 1


# ---------------------------------------------------------------- wrong twins
def test_each_rule_has_a_wrong_twin_that_a_crafted_case_catches(bow, crafted, projection):
    _, _, cases = bow
    m, nm, _ = lc.cpu_bow(cases["edges"])
    w, wn, _ = lc.cpu_bow(cases["edges"], twin="bow_le_th_low")
    assert wn == nm + 1 and m.tobytes() != w.tobytes()                  # the distance-50 pair
    w, wn, _ = lc.cpu_bow(cases["edges"], twin="bow_index_by_side2")       # KF2 has more features per node: the indices differ
    assert wn == nm and w[:len(m)].tobytes() != m.tobytes()
    w, _, _ = lc.cpu_bow(cases["tie"], twin="tie_to_later_visit")
    m, _, _ = lc.cpu_bow(cases["tie"])
    assert int(w[0]) == int(m[0]) + 1
    sc = lc.with_scale(crafted, 1.0)
    good, _ = lc.cpu_fuse(sc)
    assert not same_fuse(lc.cpu_fuse(sc, twin="fuse_keeps_chi2")[0], good)
    assert not same_fuse(lc.cpu_fuse(sc, twin="tie_to_later_visit")[0], good)
    good, _ = lc.cpu_project(projection)
    assert not same_project(lc.cpu_project(projection, twin="later_candidate_wins")[0], good)
    tied = lc.with_scale(crafted, 1.0); tied["th_proj"] = 3
    assert not same_project(lc.cpu_project(tied, twin="tie_to_later_visit")[0], lc.cpu_project(tied)[0])


# ---------------------------------------------------------------- 1-ulp scans
@pytest.mark.parametrize("kind", lc.SCAN_KINDS)
def test_scans_hold_both_outcomes(kind):
    sc = lc.scan_scene(kind)
    found = lc.scan_found(sc)
    assert len(found) == 512 and 0 < int(found.sum()) < 512
    sc["th_proj"] = int(sc.get("th", 3.0))
    assert same_fuse(lc.numpy_fuse(sc), lc.cpu_fuse(sc)[0])
    if tc.host_has_fma():
        flipped = int((lc.scan_found(sc, "fast") != found).sum())
        print("scan %s: %d of 512 decisions change under -ffp-contract=fast" % (kind, flipped))


# ---------------------------------------------------------------- random scenes
@pytest.mark.parametrize("seed", range(8))
def test_random_scw_scenes(seed):
    sc = lc.random_scw_scene(seed)
    res, _ = lc.cpu_fuse(sc)
    assert same_fuse(lc.numpy_fuse(sc), res) and sum(r[2] for r in res) > 50
    pr, br = lc.cpu_project(sc)
    assert same_project(lc.numpy_project(sc), pr) and sum(r[2] for r in pr) > 50
    assert br["already_found"] > 0 and br["target_matched"] > 0


@pytest.mark.parametrize("seed", range(8))
def test_random_bow_pairs(bow, seed):
    voc, O, _ = bow
    c = lc.random_bow_case(voc, O, seed)
    m, nm, br = lc.cpu_bow(c)
    m2, nm2 = lc.numpy_bow(c)
    assert m.tobytes() == m2.tobytes() and nm == nm2 and nm > 5
