"""CPU tests of the TrackHomo model-fit oracle (oracle/motion_oracle.inc, spec Q13) on synthetic correspondences."""
import numpy as np
import pytest

import motion_cases as mc


def _scene(rng, N, outlier_frac, noise):
    p1 = np.stack([rng.uniform(0, 1241, N), rng.uniform(0, 376, N)], 1).astype(np.float32)
    Ht = np.array([[1.02, 0.01, 6.0], [-0.005, 1.02, -3.0], [1e-5, -2e-5, 1.0]])
    q = (Ht @ np.c_[p1, np.ones(N)].T).T
    p2 = (q[:, :2] / q[:, 2:] + rng.normal(0, noise, (N, 2))).astype(np.float32)
    out = rng.random(N) < outlier_frac
    p2[out] = np.stack([rng.uniform(0, 1241, out.sum()), rng.uniform(0, 376, out.sum())], 1)
    return p1, p2, out, Ht


def test_homography_recovered_with_outliers(orc):
    rng = np.random.default_rng(3)
    p1, p2, out, Ht = _scene(rng, 900, 0.3, 0.4)
    r = orc.estimate_motion(p1, p2)
    assert r["flag"] in (1, 2) and r["n_h"] >= 0.97 * (~out).sum()
    assert r["mask_h"][~out].mean() > 0.97 and r["mask_h"][out].mean() < 0.05
    assert np.abs(r["H"] - Ht).max() < 0.1 and abs(r["H"][2, 2] - 1) < 1e-12
    # F from a planar scene is degenerate but must still be rank 2 and fit its own inliers
    assert abs(np.linalg.det(r["F"])) < 1e-12 * np.abs(r["F"]).max() ** 3 + 1e-18
    assert r["n_f"] == int(r["mask_f"].sum()) and r["n_h"] == int(r["mask_h"].sum())


def test_general_motion_prefers_fundamental(orc):
    """Points at very different depths under a sideways translation: no single homography explains them, F does."""
    rng = np.random.default_rng(4)
    N = 700
    X = np.stack([rng.uniform(-8, 8, N), rng.uniform(-2, 2, N), rng.uniform(4, 40, N)], 1)
    K = np.array([[707.0, 0, 601.9], [0, 707.0, 183.1], [0, 0, 1]])
    p1 = (K @ X.T).T; p1 = p1[:, :2] / p1[:, 2:]
    X2 = X + np.array([0.9, 0.05, -0.3])
    p2 = (K @ X2.T).T; p2 = p2[:, :2] / p2[:, 2:]
    p2 += rng.normal(0, 0.3, p2.shape)
    r = orc.estimate_motion(p1.astype(np.float32), p2.astype(np.float32))
    assert r["flag"] == 2 and r["n_f"] > 0.9 * N and r["n_h"] < r["n_f"]
    x1 = np.c_[p1, np.ones(N)]; x2 = np.c_[p2, np.ones(N)]
    l = (r["F"] @ x1.T).T
    d = np.abs(np.sum(l * x2, 1)) / np.hypot(l[:, 0], l[:, 1])
    assert np.median(d) < 1.0


def test_degenerate_inputs(orc):
    r = orc.estimate_motion(np.zeros((5, 2), np.float32), np.zeros((5, 2), np.float32))
    assert r["flag"] == 0 and r["n_h"] == 0 and r["n_f"] == 0                       # fewer than 8 pairs
    p = np.tile(np.array([[10.0, 20.0]], np.float32), (50, 1))
    r = orc.estimate_motion(p, p)
    assert r["flag"] == 0                                                          # zero spread: normalisation impossible


# ---- the crafted sets of tests/motion_cases.py reach the branches they are meant for (conditions on the INPUTS of the GPU tests)
@pytest.fixture(scope="module")
def suite_results(orc):
    return [(name, p1, p2, orc.estimate_motion_ex(p1, p2)) for name, p1, p2 in mc.suite()]


def _by_name(suite_results, name):
    hit = [r for n, _, _, r in suite_results if n == name]
    assert len(hit) == 1, name
    return hit[0]


def test_ex_entry_is_the_plain_entry(orc, suite_results):
    """orc_estimate_motion is a call to orc_estimate_motion_ex: same bytes, and the extra outputs are consistent with them."""
    for name, p1, p2, r in suite_results:
        o = orc.estimate_motion(p1, p2)
        for k in o:
            assert np.asarray(o[k]).tobytes() == np.asarray(r[k]).tobytes(), (name, k)
        assert (r["n_h"] == 0 or r["best_h"] >= 0) and (r["n_f"] == 0 or r["best_f"] >= 0), name
        assert 0 <= r["deg_h"] <= 512 and 0 <= r["deg_f"] <= 1024, name
        if r["stop_h"]:                                     # (a best count under 4 / 8 is reported as no fit: n_h / n_f = 0)
            assert 0 <= r["best_h"] < 64 and (r["n_h"] >= 0.53 * len(p1) or r["n_h"] == 0) and r["deg_h"] <= 64, name
        if r["stop_f"]:
            assert 0 <= r["best_f"] < 128 and (r["n_f"] >= 0.66 * len(p1) or r["n_f"] == 0) and r["deg_f"] <= 128, name


def test_suite_sizes():
    sizes = {len(p1) for _, p1, _ in mc.suite()}
    assert set(mc.SIZES) <= sizes
    per_size = {}
    for name, p1, _ in mc.suite():
        if name.split("-")[0] in ("planar", "general", "noise_only"):
            per_size[len(p1)] = per_size.get(len(p1), 0) + 1
    assert all(per_size[n] == len(mc.KINDS) for n in mc.SIZES)
    big = mc.suite(capacities=(2105, 5096))
    assert {2104, 2105, 5095, 5096} <= {len(p1) for _, p1, _ in big}
    assert max(len(p1) for _, p1, _ in mc.suite(capacities=(2105, 5096), max_n=2105)) == 2105
    # the same points whoever asks: a set does not depend on what else is in the list
    a = {n: (p1, p2) for n, p1, p2 in mc.suite()}
    for n, p1, p2 in big:
        if n in a:
            assert p1.tobytes() == a[n][0].tobytes() and p2.tobytes() == a[n][1].tobytes(), n
    assert all(p1.dtype == np.float32 and p2.dtype == np.float32 and p1.shape == p2.shape and p1.shape[1:] == (2,) for _, p1, p2 in big)


def test_suite_reaches_every_outcome(suite_results):
    R = [r for _, _, _, r in suite_results]
    assert any(r["flag"] == 0 for r in R) and any(r["flag"] == 1 for r in R) and any(r["flag"] == 2 for r in R)
    assert any(r["flag"] == 2 and r["n_h"] == r["n_f"] for r in R), "n_h == n_f must pick F somewhere"
    fitted = [r for r in R if r["n_h"] > 0 or r["n_f"] > 0]
    for m in ("h", "f"):
        assert any(r["stop_" + m] for r in fitted), "no set stops at the %s checkpoint" % m
        assert any(not r["stop_" + m] and r["n_" + m] > 0 for r in fitted), "no set runs the full %s hypothesis set" % m


def test_small_sets_have_degenerate_hypotheses_and_still_fit(suite_results):
    """N = 8, 9: the 8-of-N sampler can run out of its 64 draws.  The fixed seed gives planar-30%-N8 three such F hypotheses
    beside an H fit (no seed had to be changed); larger sets with singular minimal systems are collinear and scaled-1e4-0.01."""
    small = [(n, r) for n, p1, _, r in suite_results if len(p1) in (8, 9)]
    assert any(r["deg_h"] + r["deg_f"] > 0 and r["n_h"] + r["n_f"] > 0 for _, r in small)
    assert any(r["deg_h"] > 0 and r["deg_f"] > 0 and r["flag"] != 0 for _, _, _, r in suite_results)


def test_degenerate_kinds(suite_results):
    for N in mc.DEGENERATE_SIZES:
        for kind in mc.DEGENERATE_KINDS:
            r = _by_name(suite_results, "degenerate-%s-N%d" % (kind, N))
            if kind != "collinear":
                assert r["flag"] == 0 and r["n_h"] == 0 and r["n_f"] == 0, (kind, N)
                assert not r["H"].any() and not r["F"].any() and not r["mask_h"].any() and not r["mask_f"].any()
            if kind == "three_distinct":                   # the normalisation succeeds, every minimal system is singular
                assert r["deg_h"] == 512 and r["deg_f"] == 1024
    # collinear is ill-conditioned, not refused: a line under a translation is fitted by H; only GPU == oracle is asked of it
    r = _by_name(suite_results, "degenerate-collinear-N50")
    assert (r["flag"], r["n_h"], r["n_f"]) == (1, 50, 0) and r["deg_h"] > 256


def test_the_more_than_ten_rule(suite_results):
    a10, a11 = _by_name(suite_results, "all_inliers-N10"), _by_name(suite_results, "all_inliers-N11")
    assert (a10["flag"], a10["n_h"], a10["n_f"]) == (0, 10, 0)
    assert (a11["flag"], a11["n_h"], a11["n_f"]) == (1, 11, 0)
    for N in mc.ALL_INLIERS_SIZES:                          # every F hypothesis of a pure translation is degenerate
        r = _by_name(suite_results, "all_inliers-N%d" % N)
        assert r["n_h"] == N and r["n_f"] == 0 and r["deg_f"] == 1024 and r["best_f"] == -1, N
    for N, flag in ((8, 0), (9, 0), (10, 0), (11, 2), (20, 2)):
        r = _by_name(suite_results, "planar-0%%-N%d" % N)
        assert (r["flag"], r["n_h"], r["n_f"]) == (flag, N, N), N
    for N in (0, 1, 7):
        for kind, frac in mc.KINDS:
            r = _by_name(suite_results, "%s-%s-N%d" % (kind, "%d%%" % round(100 * frac) if frac is not None else "x", N))
            assert r["flag"] == 0 and r["n_h"] == 0 and r["n_f"] == 0 and r["best_h"] == -1 and r["best_f"] == -1


def test_checkpoint_edges(suite_results):
    """exact_share: the best H count is n_in exactly; 0.53 N lies between n_in = 52 and 53 of 100, 105 and 106 of 200."""
    for N, n_in in mc.EXACT_SHARES:
        r = _by_name(suite_results, "exact_share-N%d-%d" % (N, n_in))
        assert r["n_h"] == n_in and r["stop_h"] == (n_in >= 0.53 * N), (N, n_in)
    # by outlier share: 30 % stops both searches, 55 % runs both to the end
    for N in (257, 1000, 2049, 4097):
        a, b = _by_name(suite_results, "planar-30%%-N%d" % N), _by_name(suite_results, "planar-55%%-N%d" % N)
        assert a["stop_h"] and a["stop_f"] and not b["stop_h"] and not b["stop_f"], N


def test_refit_chunks_and_count_passes(suite_results):
    """H inlier sets that end in the second and the third 256-pair chunk of the refit and beyond one 2048-pair pass of the
    count, with inliers and outliers on both sides of index 256 (the inliers are not contiguous)."""
    def mixed(r):
        m = r["mask_h"]
        return 0 < m[:256].sum() < 256 and 0 < m[256:].sum() < len(m) - 256
    R = [r for _, _, _, r in suite_results]
    assert any(256 < r["n_h"] <= 512 and mixed(r) for r in R)
    assert any(512 < r["n_h"] <= 768 and mixed(r) for r in R)
    assert any(r["n_h"] > 2048 and mixed(r) for r in R)
    assert sum(len(r["mask_h"]) > 2048 and r["flag"] != 0 for r in R) >= 10
