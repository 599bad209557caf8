"""The PnPsolver CPU oracle (tests/cpp/pnp_oracle.cpp) and the crafted problems of tests/pnp_cases.py, without a GPU: every case reaches
the branch it was made for and keeps its decision under both summation orders and both contraction settings, every deliberately wrong
twin differs on the case built for it, the sampler's sparse form equals the literal vector, the one SVD routine and the EPnP pipeline
agree with numpy, and SetRansacParameters keeps its quirks."""
import itertools

import numpy as np
import pytest

import pnp_cases as pc


@pytest.fixture(scope="module")
def results():
    return [(pr, *pc.iterate(pr)) for pr in pc.ransac_cases()]


def test_every_case_reaches_its_branch(results):
    names = [pr["name"] for pr, *_ in results]
    assert len(set(names)) == len(names)
    for pr, r, inl, info in results:
        name, ex = pr["name"], pr["expect"]
        N = len(pr["corr"])
        end = pc.end_of(pr, r)
        assert r["kind"] in (0, 1, 2) and r["max_its"] >= 1 and r["min_inliers"] >= 4, name
        assert r["no_more"] == (0 if r["kind"] == 1 else 1), name
        if r["kind"] == 1:
            assert r["n_inliers"] > r["min_inliers"] and int(inl.sum()) == r["n_inliers"], name           # PnP:292 is strict
            assert pr["prob"]["start_iteration"][0] < r["iteration"] <= end and 1 <= r["best_iteration"] <= r["iteration"], name
            assert r["best_inliers"] >= r["min_inliers"] and r["n_refines"] >= 1, name
        elif r["kind"] == 2:
            assert r["iteration"] == end and r["n_inliers"] == r["best_inliers"] >= r["min_inliers"] and int(inl.sum()) == r["n_inliers"], name
        else:
            assert not inl.any() and not r["Tcw"].any() and r["n_inliers"] == 0 and r["best_iteration"] == 0, name
            assert r["iteration"] == end, name
        assert info["iterations"] == r["iteration"], name
        for k in ("kind", "iteration", "max_its"):
            if k in ex:
                assert r[k] == ex[k], (name, k, r[k])
        if "iterations" in ex:
            assert info["iterations"] == ex["iterations"], name
        if ex.get("at_end"):
            assert r["iteration"] == end == r["max_its"], name
        if ex.get("ties"):
            assert info["ties"] > 0, name
        if ex.get("below_min"):
            assert info["below_min"] > 0 and r["best_inliers"] == 0, name
        if "refined" in ex:
            assert r["n_inliers"] == ex["refined"] == (r["min_inliers"] if r["kind"] == 2 else r["min_inliers"] + 1), name
        if ex.get("refine_fails"):
            assert info["refine_fails"] >= 1, name
        if "flag" in ex:
            assert info["hyp_flags"] & ex["flag"], name
        if "outside" in ex:
            assert inl[ex["outside"]] == 0 and r["n_inliers"] == N - 1, name
    kinds = {int(r["kind"]) for _, r, _, _ in results}
    assert kinds == {0, 1, 2}


def test_named_cases(results):
    by = {pr["name"]: (pr, r, inl, info) for pr, r, inl, info in results}
    pr, r, inl, info = by["size_4_min4"]                  # mRansacMinInliers == N: nIterations = 1, and yet iterate(5) runs five
    assert (r["max_its"], r["min_inliers"], r["iteration"], r["best_iteration"]) == (1, 4, 5, 1) and info["refine_calls"] == info["ties"] + 1
    assert by["size_%d" % pc.MAX_N][1]["n_inliers"] > 2048
    pr, r, inl, info = by["decoy_then_true"]
    assert r["n_refines"] == 2 and r["best_iteration"] == r["iteration"] and not inl[pr["bad"]].any() and inl[~pr["bad"]].all()
    pr, r, inl, info = by["resume_same_best"]
    first = pc.iterate(pr["first_call"])[0]
    assert pr["prob"]["start_iteration"][0] == first["iteration"] and r["best_iteration"] == first["best_iteration"] <= first["iteration"] < r["iteration"]
    pr, r, inl, info = by["resume_new_best"]
    first = pc.iterate(pr["first_call"])[0]
    assert r["best_iteration"] > first["iteration"] == pr["prob"]["start_iteration"][0] and r["best_inliers"] > first["best_inliers"]
    for name in ("outliers_30", "outliers_60", "found_middle", "found_at_end"):
        pr, r, inl, info = by[name]
        assert not inl[pr["bad"]].any() and r["kind"] == 1, name
    pr, r, inl, info = by["found_middle"]
    assert 3 <= r["iteration"] < r["max_its"]
    # every branch of the beta approximations, the sign flip and the reflection is reached somewhere, and each approximation wins somewhere
    flags = 0
    wins = np.zeros(3, np.int64)
    for pr, r, inl, info in results:
        flags |= info["hyp_flags"] | info["refine_flags"]
        wins += [info["win1"], info["win2"], info["win3"]]
    assert flags == pc.F_B4_NEG | pc.F_B4_ZERO | pc.F_B3_1_NEG | pc.F_SIGN | pc.F_DET and (wins > 0).all()


def test_decisions_hold_under_both_orders_and_contractions(results):
    """What lets the GPU tests compare decisions exactly: none of the crafted cases sits on an edge that the summation order or FMA moves."""
    for pr, r, inl, info in results:
        assert pc.stable(pr), pr["name"]


def test_recorded_spread_covers_the_oracles_own(results):
    """profiles/pnp_tolerance.json is what tests/test_gpu_pnp.py bounds the device's pose with: one entry per crafted case, and the spread
    recomputed here (both orders, both contraction settings) does not exceed the recorded one."""
    import json
    import os
    tol = json.load(open(os.path.join(pc.ROOT, "profiles", "pnp_tolerance.json")))["cases"]
    assert set(tol) == {pr["name"] for pr, *_ in results}
    for pr, *_ in results:
        assert pc.spread(pr) <= tol[pr["name"]]["spread"] <= 1e-5, pr["name"]


def test_each_twin_differs_on_its_case(results):
    by = {pr["name"]: (pr, r) for pr, r, _, _ in results}
    for twin, name in (("refine_ge", "count_equals_min"), ("best_ge", "count_equals_min"), ("best_ge", "size_4_min4"),
                       ("refine_current", "refine_takes_best_mask"), ("loop_and", "size_4_min4"), ("loop_and", "found_at_end"),
                       ("err_le", "bound_scan"), ("pow4", "outliers_60")):
        pr, r = by[name]
        assert not pc.same_result(pc.iterate(pr, twin=twin)[0], r), (twin, name)
    pr, r = by["count_equals_min"]
    assert pc.iterate(pr, twin="refine_ge")[0]["kind"] == 1 and r["kind"] == 2                           # >= would accept exactly min_inliers
    assert pc.iterate(pr, twin="best_ge")[0]["best_iteration"] > r["best_iteration"]                     # >= keeps the latest of equal counts
    pr, r = by["size_4_min4"]
    assert pc.iterate(pr, twin="loop_and")[0]["iteration"] == 1                                           # && stops at mRansacMaxIts = 1


def test_bound_scan_holds_both_outcomes(results):
    pr = next(p for p, *_ in results if p["name"] == "bound_scan")
    cnt, poses, masks = pc.hypotheses(pr, 1)
    scan = pr["scan"]
    assert scan.sum() == 512 and np.array_equal(masks[0][scan], pr["scan_want"][scan])
    assert 0 < pr["scan_want"][scan].sum() < 512 and masks[0][pr["equal_item"]] == 0
    rows = pc.rows_of(pr)
    K = pr["prob"]["K"][0]
    for i in np.nonzero(scan)[0][:64]:                      # one f32 step of uv[0] flips the decision, at every octave
        r2 = rows[i:i + 1].copy()
        r2[0, 3] = np.nextafter(r2[0, 3], np.float32(np.inf) if pr["scan_want"][i] else np.float32(-np.inf))
        assert pc.check(poses[0], r2, K)[0] == 1 - pr["scan_want"][i]
    assert len(set(np.round(rows[scan, 5], 3))) == 8


def test_sampler_sparse_form_equals_the_literal_vector():
    for N in range(4, 9):
        seen = set()
        for seed, it in itertools.product(range(40), range(1, 40)):
            a, b = pc.sample_literal(seed, it, N), pc.sample_closed(seed, it, N)
            assert np.array_equal(a, b), (N, seed, it)
            assert len(set(a.tolist())) == 4 and a.min() >= 0 and a.max() < N
            seen.add(tuple(a.tolist()))
        assert len(seen) == N * (N - 1) * (N - 2) * (N - 3) or N > 5           # every ordered draw occurs for the small sizes
    for N in (9, 100, 4096):
        for it in (1, 2, 4095, 4096):
            assert np.array_equal(pc.sample_literal(12345, it, N), pc.sample_closed(12345, it, N))


def _parameters(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, exponent=3):
    """PnP:121-157 restated in numpy scalars (float32 where the reference has float)."""
    n_min = max(int(np.float32(N) * np.float32(epsilon)), min_inliers, min_set)
    eps = np.float32(epsilon)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float32(n_min) / np.float32(N)
        if eps < ratio:
            eps = ratio
        if n_min == N:
            its = 1
        else:
            v = np.ceil(np.log(1 - probability) / np.log(1 - np.float64(eps) ** exponent))
            its = max_iterations if not v < max_iterations else max(int(v), 1)
    return n_min, max(1, min(its, max_iterations))


def test_set_ransac_parameters_keeps_its_quirks():
    assert pc.ransac_parameters(100) == (50, 35)                       # int(N * epsilon); ceil(log(0.01) / log(1 - 0.5^3)) = 35, exponent 3
    assert pc.ransac_parameters(100, twin="pow4")[1] == 72             # what the exponent 4 of the minimal set would give
    assert pc.ransac_parameters(15) == (10, 14)                        # the epsilon raise to 10 / 15: ceil(4.605 / 0.3514)
    assert pc.ransac_parameters(10) == (10, 1)                         # mRansacMinInliers == N -> 1
    assert pc.ransac_parameters(3) == (10, 300)                        # N < min_inliers: epsilon > 1, the log is NaN, clamped to max_iterations
    assert pc.ransac_parameters(0) == (10, 300)
    assert pc.ransac_parameters(7, min_inliers=2)[0] == 4              # the minimal set is the floor
    assert pc.ransac_parameters(4096, epsilon=0.001, min_inliers=4)[1] == 300
    assert pc.ransac_parameters(101, epsilon=0.5)[0] == 50             # through float, truncated
    for N in list(range(0, 70)) + [100, 101, 1023, 4096]:
        for kw in (dict(), dict(min_inliers=2), dict(epsilon=0.3), dict(epsilon=1.0), dict(probability=0.5, max_iterations=7), dict(epsilon=0.01, min_inliers=4)):
            assert pc.ransac_parameters(N, **kw) == _parameters(N, **kw), (N, kw)
            assert pc.ransac_parameters(N, twin="pow4", **kw) == _parameters(N, exponent=4, **kw), (N, kw)


def test_svd_routine_against_numpy():
    rng = np.random.default_rng(5)
    for m, n in ((3, 3), (6, 3), (6, 4), (6, 5), (12, 12)):
        A = rng.normal(size=(m, n))
        U, w, V = pc.svd(A)
        assert np.all(np.diff(w) <= 0) and np.abs(w - np.linalg.svd(A, compute_uv=False)).max() < 1e-13
        assert np.abs((U * w) @ V.T - A).max() < 1e-13 and np.abs(V.T @ V - np.eye(n)).max() < 1e-13 and np.abs(U.T @ U - np.eye(n)).max() < 1e-13
    M = rng.normal(size=(8, 12))                                        # the 4-point case: a 4-dimensional null space, read from V
    U, w, V = pc.svd(M.T @ M)
    assert np.abs(w[8:]).max() < 1e-12 * w[0] and np.abs(M @ V[:, 8:]).max() < 1e-12 and np.abs(V.T @ V - np.eye(12)).max() < 1e-13
    U, w, V = pc.svd(np.zeros((3, 3)))                                  # zero singular values: U's column is zero, V stays orthonormal
    assert not w.any() and not U.any() and np.array_equal(V, np.eye(3))
    U, w, V = pc.svd(np.diag([2.0, 5.0, 5.0]))                          # sorted descending, the first of equal values first
    assert w.tolist() == [5.0, 5.0, 2.0] and V[:, 0].tolist() == [0, 1, 0] and V[:, 1].tolist() == [0, 0, 1]


def test_epnp_against_numpy_and_the_true_pose():
    """Well-conditioned, noise-free scenes: the oracle's pose equals the true pose and the numpy / float64 restatement (numpy.linalg.svd,
    lstsq, pinv) to 1e-6 -- far above f64 round-off through EPnP's squared systems, far below any modelling difference."""
    for seed, n in ((1, 6), (2, 12), (3, 100), (4, 1000)):
        pr = pc.make_problem(seed, n, depth=(4.0, 12.0))
        rows = pc.rows_of(pr)
        K = pr["prob"]["K"][0]
        for order in (0, 1):
            R, t, ex = pc.pose(rows, K, order)
            Rn, tn, _ = pc.epnp_numpy(rows[:, :3], rows[:, 3:5], K)
            assert np.abs(R - Rn).max() < 1e-6 and np.abs(t - tn).max() < 1e-6, (seed, n, order)
            assert np.abs(R - pr["R"]).max() < 1e-5 and np.abs(t - pr["t"]).max() < 1e-4, (seed, n, order)
            assert abs(np.linalg.det(R) - 1) < 1e-9 and ex["rep"].min() < 1e-3


def test_refine_stage_in_both_orders():
    pr = next(p for p in pc.ransac_cases() if p["name"] == "size_%d" % pc.MAX_N)
    r = pc.iterate(pr)[0]
    cnt, poses, masks = pc.hypotheses(pr, int(r["best_iteration"]))
    rows, K = pc.rows_of(pr), pr["prob"]["K"][0]
    n0, p0, m0 = pc.refine(rows, masks[-1], K, order=0)
    n1, p1, m1 = pc.refine(rows, masks[-1], K, order=1)
    assert n0 == n1 == r["n_inliers"] and np.array_equal(m0, m1)
    assert p0.tobytes() != p1.tobytes() and np.abs(p0 - p1).max() < 1e-9      # the order moves the last bits of the f64 pose, nothing else
    assert np.array_equal(p0[:9].astype(np.float32), r["Tcw"].reshape(4, 4)[:3, :3].reshape(-1))
