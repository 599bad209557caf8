"""The Sim3Solver CPU oracle (tests/cpp/sim3_oracle.cpp) and the crafted problems of tests/sim3_cases.py, without a GPU: every case
reaches the branch it was made for, the sampler's closed form equals the literal vector, the error-bound scans hold both outcomes,
and clean problems recover their similarity."""
import itertools
import json
import os

import numpy as np
import pytest

import sim3_cases as sc

TOL_PATH = os.path.join(sc.ROOT, "profiles", "sim3_tolerance.json")
SCAN_GEOMETRIES, SCAN_POINTS = 16, 32


@pytest.fixture(scope="module")
def results():
    return [(pr, *sc.find(pr)) for pr in sc.ransac_cases()]


def test_every_case_reaches_its_branch(results):
    seen = set()
    for pr, r, inl, info in results:
        name, what = pr["name"], pr["expect"]
        br = sc.BRANCH[int(info[0])]
        seen.add(br)
        assert r["max_its"] >= 1, name
        if br == "none":
            assert (r["found"], r["no_more"], r["iteration"], r["n_inliers"]) == (0, 1, 0, 0) and info[1] == 0 and not inl.any(), name
            assert not np.asarray(r["T12"]).any(), name
        elif br == "found":
            assert r["found"] == 1 and r["no_more"] == 0 and r["n_inliers"] > pr["min_inliers"] and int(inl.sum()) == r["n_inliers"], name
            assert info[1] == r["iteration"] <= r["max_its"], name              # the sequential loop stopped there
        else:
            assert r["found"] == 0 and r["no_more"] == 1 and r["n_inliers"] <= pr["min_inliers"] and not inl.any(), name
            assert info[1] == r["max_its"], name
        if what is None:
            continue
        assert {"found_first": "found", "found_last": "found"}.get(what, what) == br, (name, what, br)
        if what == "found_first":
            assert r["iteration"] == 1, name
        if what == "found_last":
            assert r["iteration"] == r["max_its"] == pr["max_iterations"], name
    assert seen == {"none", "found", "exhausted"}


def test_named_cases(results):
    by = {pr["name"]: (pr, r, inl, info) for pr, r, inl, info in results}
    assert by["size_20"][1]["max_its"] == 1 and by["min_inliers_equals_n"][1]["max_its"] == 1          # mRansacMinInliers == N: nIterations = 1
    assert by["size_%d" % sc.MAX_N][1]["n_inliers"] == sc.MAX_N
    pr, r, inl, info = by["all_outliers"]
    assert info[2] > 0, "no later hypothesis tied the best count: the >= rule is not exercised"
    assert r["iteration"] > 1
    pr, r, inl, info = by["coincident"]
    assert info[3] == info[1] and r["n_inliers"] == 0 and r["iteration"] == r["max_its"]               # 0 / 0 scale: nothing is an inlier, the latest stays
    assert not np.isfinite(r["s12"])
    pr, r, inl, info = by["z_zero"]
    assert inl[5] == 0 and inl[6] == 0 and r["n_inliers"] == 38
    pr, r, inl, info = by["outliers_30"]
    assert r["iteration"] >= 1 and not inl[pr["bad"]].any() and inl[~pr["bad"]].all()
    pr, r, inl, info = by["outliers_60"]
    assert not inl[pr["bad"]].any() and r["n_inliers"] > 20
    for s in (0.5, 1.0, 2.0):
        pr, r, inl, info = by["clean_s%g_fix0" % s]
        assert r["n_inliers"] == len(inl) and abs(float(r["s12"]) / s - 1) < 1e-3
        pr, r, inl, info = by["clean_s%g_fix1" % s]
        assert r["s12"] == 1.0 and (r["found"] == 1) == (s == 1.0)


def test_error_bound_is_truncated(results):
    """mvnMaxError is a vector of size_t: level 0 admits err < 9, not err < 9.21."""
    pr, r, inl, info = next(x for x in results if x[0]["name"] == "error_bound")
    I = np.eye(4, dtype=np.float32)
    assert np.array_equal(np.asarray(r["T12"]).reshape(4, 4), I) and r["iteration"] == 1
    _, err, _ = sc.check(pr, I, I)
    rows = pr["probes"]
    assert 8.85 < err[rows[8.9], 0] < 8.95 and inl[rows[8.9]] == 1
    assert 9.05 < err[rows[9.1], 0] < 9.15 and inl[rows[9.1]] == 0                    # inside 9.21, outside (size_t)9.21
    assert 9.15 < err[rows[9.2], 0] < 9.21 and inl[rows[9.2]] == 0
    assert 8.99 < err[rows[9.0], 0] < 9.01 and inl[rows[9.0]] == int(err[rows[9.0], 0] < np.float32(9.0))
    assert inl[:25].all()


def test_closed_form_sampler_equals_the_literal_vector():
    n = 0
    for N in range(3, 9):
        for r in itertools.product(range(N), range(N - 1), range(N - 2)):
            assert sc.removal_closed_form(r, N) == sc.removal_literal(list(r), N), (N, r)
            n += 1
    assert n == sum(N * (N - 1) * (N - 2) for N in range(3, 9))
    for seed, it, N in ((0, 1, 3), (1, 300, 150), (2 ** 63 + 5, 4096, 4096), (12345, 7, 4)):
        got = sc.removal_closed_form(sc.draws(seed, it, N), N)
        assert got == sc.sample_literal(seed, it, N) and len(set(got)) == 3


def test_max_iterations_formula():
    f = sc.oracle().sd_sim3_oracle_max_its
    assert f(0.99, 20, 300, 20) == 1
    assert f(0.99, 20, 300, 21) == 3                                   # ceil(log(0.01) / log(1 - (20/21)^3)) = ceil(2.33)
    assert f(0.99, 20, 300, 150) == 300
    assert f(0.99, 20, 300, 40) == int(np.ceil(np.log(0.01) / np.log(1 - np.float64(np.float32(20) / np.float32(40)) ** 3)))
    assert f(0.99, 20, 300, 0) >= 1 and f(0.99, 20, 300, 5) >= 1 and f(0.99, 1, 300, 4000) == 300


def _scans():
    out = []
    for g in range(SCAN_GEOMETRIES):
        pr, row, vals = sc.bound_scan(g, SCAN_POINTS)
        out.append((pr, row, vals))
    return out


def test_error_bound_scans_hold_both_outcomes(capsys):
    I = np.eye(4, dtype=np.float32)
    changed = total = 0
    for pr, row, vals in _scans():
        dec, fast = [], []
        for v in vals:
            pr["corr"]["xw2"][row][0] = v
            dec.append(int(sc.check(pr, I, I)[2][row])); fast.append(int(sc.check(pr, I, I, contract="fast")[2][row]))
        assert 0 < sum(dec) < len(dec), "a scan must hold both outcomes"
        k = dec.index(0)
        assert all(dec[:k]) and not any(dec[k:]), "one crossing per scan"
        changed += sum(a != b for a, b in zip(dec, fast)); total += len(dec)
    with capsys.disabled():
        print("\nsim3 error-bound scans: %d of %d decisions change with -ffp-contract=fast" % (changed, total))
    assert total == SCAN_GEOMETRIES * SCAN_POINTS


def _horn_deviation():
    """Largest deviation of the oracle's ComputeSim3 from a float64 numpy Horn solve on the same three f32 points, over the winning
    samples of the clean cases: (entries of T12 relative to max(1, |entry|), relative scale)."""
    dT = ds = 0.0
    for pr in sc.ransac_cases():
        if not pr["name"].startswith("clean_") or pr["name"].endswith("fix1") and pr["truth"][0] != 1.0:
            continue
        r, _, _ = sc.find(pr)
        c, p = pr["corr"], pr["prob"]
        idx = sc.sample_literal(int(p["seed"]), int(r["iteration"]), len(c))
        T1 = np.asarray(p["Tcw1"], np.float64).reshape(4, 4); T2 = np.asarray(p["Tcw2"], np.float64).reshape(4, 4)
        x1 = (c["xw1"][idx].astype(np.float64) @ T1[:3, :3].T + T1[:3, 3]).astype(np.float32)
        x2 = (c["xw2"][idx].astype(np.float64) @ T2[:3, :3].T + T2[:3, 3]).astype(np.float32)
        fix = bool(p["fix_scale"])
        h = sc.horn(x1, x2, fix)
        s, R, t = sc.horn_f64(x1, x2, fix)
        T = np.eye(4); T[:3, :3] = s * R; T[:3, 3] = t
        dT = max(dT, float(np.max(np.abs(h["T12"].astype(np.float64) - T) / np.maximum(1.0, np.abs(T)))))
        ds = max(ds, abs(float(h["s"]) / s - 1))
        assert np.allclose(h["T12"].astype(np.float64) @ h["T21"].astype(np.float64), np.eye(4), atol=1e-4)
    return dT, ds


def test_clean_cases_recover_the_similarity():
    for pr in sc.ransac_cases():
        if not pr["name"].startswith("clean_"):
            continue
        r, inl, _ = sc.find(pr)
        s, R, t = pr["truth"]
        if r["found"]:
            assert r["n_inliers"] == len(inl)
            T = np.eye(4); T[:3, :3] = s * R; T[:3, 3] = t
            # three points a few metres apart at 5-25 m carry f32 rounding of ~1e-6 relative; the lever arm of the sample stays below 1e3
            assert np.max(np.abs(np.asarray(r["T12"], np.float64).reshape(4, 4) - T)) < 2e-3, pr["name"]
    dT, ds = _horn_deviation()
    rec = json.load(open(TOL_PATH))
    assert dT <= 10 * rec["horn_vs_f64"]["T12"] and ds <= 10 * rec["horn_vs_f64"]["s12"], (dT, ds, rec)


# ---------------------------------------------------------------- SearchBySim3
def test_search_scene_reaches_every_branch():
    s = sc.crafted_search_scene()
    res, cnt = sc.cpu_search(s)
    sc.check_search_expectations(s, res)
    m12, v1, v2, nf, b1, b2 = res[0]
    for d, b in ((0, b1), (1, b2)):
        seen = {sc.S3_BRANCHES[int(x)] for x in b}
        assert seen >= set(sc.S3_BRANCHES) - {"not_finite"}, (d, set(sc.S3_BRANCHES) - seen)
    assert cnt["octave_below"] >= 2 and cnt["octave_above"] >= 2 and cnt["octave_lm1"] >= 2 and cnt["tie"] >= 2 and cnt["window_max"] == 65
    i1, i2 = s["agree"]
    assert m12[i1] == i2 and nf == 1 and cnt["agree_ok"] == 1                       # the one pair the function adds
    assert v1[s["disagree"]] >= 0 and m12[s["disagree"]] == -1 and cnt["agree_fail"] >= 1
    assert abs(s["pairs"][0]["s12"] - 1) > 0.2


@pytest.mark.parametrize("cols", [16, 17])
def test_search_window_columns(cols):
    s = sc.wide_window_scene(cols)
    res, cnt = sc.cpu_search(s)
    sc.check_search_expectations(s, res)
    assert cnt["cols_max"] == cols


def test_search_scans_hold_both_outcomes(capsys):
    report = {}
    for kind in sc.SEARCH_SCAN_KINDS:
        s, rows = sc.search_scan_scene(kind)
        res, _ = sc.cpu_search(s)
        fast, _ = sc.cpu_search(s, contract="fast")
        changed = total = 0
        for q, (d, feats, code) in enumerate(rows):
            dec = [int(res[q][4 + d][f]) == code for f in feats]
            alt = [int(fast[q][4 + d][f]) == code for f in feats]
            assert 0 < sum(dec) < len(dec), (kind, q)
            k = dec.index(True)
            assert not any(dec[:k]) and all(dec[k:]), (kind, q, "one crossing per scan")
            changed += sum(a != b for a, b in zip(dec, alt)); total += len(dec)
        assert total == sc.SEARCH_SCAN_GEOMETRIES * sc.SEARCH_SCAN_POINTS
        report[kind] = changed
    with capsys.disabled():
        print("\nSearchBySim3 scans, decisions that change with -ffp-contract=fast (of %d each): %r" % (total, report))


def test_random_search_scene_is_busy():
    s = sc.random_search_scene(3, 300, 2)
    res, cnt = sc.cpu_search(s)
    assert all(r[3] > 20 for r in res) and cnt["agree_fail"] > 20 and cnt["octave_below"] > 50 and cnt["octave_above"] > 50
