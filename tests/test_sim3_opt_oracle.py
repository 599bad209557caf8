"""The OptimizeSim3 CPU oracle (tests/cpp/sim3_opt_oracle.cpp) and the crafted problems of tests/sim3_opt_cases.py, without a GPU:
every case reaches the branch it was made for, a plain numpy restatement agrees on the objective and on the Jacobian, every wrong
twin differs somewhere, the chi2 decisions keep their margin, the recorded spreads are reproduced, the private sin / cos / exp stay
within one ulp of the C library, and the C ABI refuses what it must before anything is launched."""
import json
import os
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as sc

TOL_PATH = os.path.join(sc.ROOT, "profiles", "sim3_opt_tolerance.json")
CHI2_MARGIN = 1e-6          # DESIGN Q37's margin, carried over for the decisions that have one (Q45)


@pytest.fixture(scope="module")
def cases():
    return sc.crafted_cases()


@pytest.fixture(scope="module")
def runs(cases):
    return {c["name"]: (c, *sc.solve(c)) for c in cases}


@pytest.fixture(scope="module")
def wave_runs(cases):
    return {c["name"]: (c, *sc.solve(c, sc.WAVE)) for c in cases}


def test_every_case_reaches_what_it_was_made_for(runs):
    for name, (c, r, st, info, mg) in runs.items():
        e = c["expect"]
        assert r["n_correspondences"] == len(c["corr"]), name
        assert r["more_iterations"] == (10 if r["n_bad"] > 0 else 5), name
        assert r["written"] == int(len(c["corr"]) - r["n_bad"] >= 10), name
        assert int((st == 1).sum()) == r["n_bad"], name
        if r["written"]:
            assert r["ret"] == int((st == 0).sum()), name
        else:                                                   # return 0: the prior comes back, the NULLed matches stay
            assert r["ret"] == 0 and not (st == 2).any() and r["iterations"][1] == 0, name
            assert np.allclose(sc.quat_to_R(r["q"]), np.asarray(c["prob"]["R12"], np.float64).reshape(3, 3), atol=1e-6), name
            assert np.array_equal(r["t"], np.asarray(c["prob"]["t12"], np.float64)) and r["s"] == float(c["prob"]["s12"]), name
        for key, field in (("ret", "ret"), ("n_bad", "n_bad"), ("more", "more_iterations"), ("written", "written")):
            if key in e:
                assert r[field] == e[key], (name, key, r[field], e[key])
        if "stop0" in e:
            assert r["stop"][0] == e["stop0"] and r["iterations"][0] == e["iterations0"], name
        if "solve_failed" in e:
            assert (info[sc.I_SOLVE_FAILED] > 0) == bool(e["solve_failed"]), name
        if "branch" in e:
            assert info[sc.I_BRANCH0 + e["branch"]] > 0, name
        if "fix" in e and e["fix"]:
            assert r["s"] == float(c["prob"]["s12"]) and info[sc.I_BRANCH0 + 2] == 0 and info[sc.I_BRANCH0 + 3] == 0, name
        if "bad" in c and c["exact"] and r["written"] and c["bad"].any() and r["n_bad"] == c["bad"].sum():
            assert (st[c["bad"]] == 1).all(), name              # the planted outliers are the ones removed


def test_the_set_covers_every_path(runs, wave_runs):
    for which in (runs, wave_runs):
        rs = [x[1] for x in which.values()]
        infos = np.array([x[3] for x in which.values()])
        assert {int(s) for r in rs for s in r["stop"]} == {sc.STOP_OK, sc.STOP_TRIALS, sc.STOP_RHO_ZERO, sc.STOP_NO_GAIN}
        assert all(infos[:, sc.I_BRANCH0 + b].sum() > 0 for b in range(4)), "a Sim3(update) branch is not reached"
        assert {int(r["more_iterations"]) for r in rs} == {5, 10}
        assert {r["ret"] >= 20 for r in rs if r["written"]} == {True, False}
        assert infos[:, sc.I_SOLVE_FAILED].sum() > 0 and infos[:, sc.I_HUBER].sum() > 0 and infos[:, sc.I_NONFINITE].sum() > 0
    c, r, st, info, mg = runs["z_zero"]
    assert info[sc.I_LAST_REJECTED_R1] == 1 and info[sc.I_STALE_R1] > 0, "the stale _error of a rejected last trial must decide a flag"
    assert r["n_bad"] == 0 and r["ret"] == len(st) and sc.solve(c, sc.TWIN_RECOMPUTE)[0]["n_bad"] > 0
    # the rank-deficient sets do NOT make isPositive() fail: H is a sum of J^T W J with W > 0 and lambda I is added to it
    for name in ("one_point_repeated", "points_on_a_line"):
        assert runs[name][3][sc.I_SOLVE_FAILED] == 0, name
    assert runs["behind_camera"][1]["ret"] == 30 and (sc.camera_points(runs["behind_camera"][0])[0][:3, 2] < 0).all()


def test_every_wrong_twin_differs_on_a_crafted_case(cases, runs):
    for twin, flag in sc.TWINS.items():
        differing = []
        for c in cases:
            r, st = sc.solve(c, flag)[:2]
            if r.tobytes() != runs[c["name"]][1].tobytes() or st.tobytes() != runs[c["name"]][2].tobytes():
                differing.append(c["name"])
        assert differing, twin
    # the decisions, not only the bits: the twins that change a count
    assert sc.solve(runs["outliers_in_kf2_only"][0], sc.TWIN_SINGLE_CHI2)[0]["n_bad"] == 0
    assert sc.solve(runs["far_prior_all_bad"][0], sc.TWIN_WRITE_ON_ZERO)[0]["written"] == 1


def test_numpy_restatement_agrees(runs):
    for name, (c, r, st, info, mg) in runs.items():
        n = len(c["corr"])
        if n == 0 or not c["exact"] or name == "negative_information":
            continue
        est = np.concatenate([r["q"], r["t"], [r["s"]]])
        E = sc.np_errors(c, est)
        for i in sorted({0, n // 2, n - 1}):
            Jn, Ja, err = sc.jacobians(c, i, est)
            assert np.allclose(err, E[i], rtol=1e-9, atol=1e-9), (name, i)
            Jp = sc.np_analytic_jacobian(c, i, est)
            scale = np.abs(Jp).max()
            # delta = 1e-9 central differences: truncation plus the cancellation of two ~100 px errors, 1e-5 relative (not tuned)
            assert np.abs(Jn - Jp).max() <= 1e-5 * scale and np.abs(Ja - Jp).max() <= 1e-9 * scale, (name, i)
        if r["written"]:                                        # the estimate is a minimum of the robust objective over the inliers of round 1
            live = st != 1
            f0 = sc.np_objective(c, est, live)
            for d in range(6 if int(c["prob"]["fix_scale"]) else 7):
                for sign in (1e-3, -1e-3):
                    u = np.zeros(7); u[d] = sign
                    moved, _ = sc.oplus(est, u, 0)
                    assert sc.np_objective(c, moved, live) >= f0 * (1 - 1e-3), (name, d, sign)


def test_numpy_objective_equals_the_oracles_on_every_case(runs):
    for name, (c, r, st, info, mg) in runs.items():
        n = len(c["corr"])
        prior = np.concatenate([sc.solve(dict(c, corr=c["corr"][:0]))[0][f].reshape(-1) for f in ("q", "t", "s")])     # Sim3(R12, t12, s12)
        for est, live in ((prior, np.ones(n, bool)), (np.concatenate([r["q"], r["t"], [r["s"]]]), st != 1)):
            a, b = sc.objective(c, est, live), sc.np_objective(c, est, live)
            if a != a or b != b:
                assert a != a and b != b, (name, a, b)          # z_zero: NaN on both sides
            else:
                assert a == pytest.approx(b, rel=1e-9, abs=1e-12), (name, a, b)


def test_the_estimate_is_bitwise_the_same_with_the_scale_column_dropped(cases, runs):
    """The variant the issue lists as a sixth wrong twin is not wrong: with _fix_scale the seventh row and column of H are exact zeros
    plus lambda, uncoupled from the other six unknowns, so a 6 x 6 system gives the same bits.  Asserted, not argued."""
    n = 0
    for c in cases:
        r, st = sc.solve(c, sc.DROP_SCALE)[:2]
        same = all(np.array_equal(np.asarray(r[f]), np.asarray(runs[c["name"]][1][f]), equal_nan=np.asarray(r[f]).dtype.kind == "f") for f in sc.RESULT_DTYPE.names)
        assert same and np.array_equal(st, runs[c["name"]][2]), c["name"]
        n += int(c["prob"]["fix_scale"]) and len(c["corr"]) >= 10
    assert n >= 2
    for k in range(40):                                         # and on the fuzz's fixed-scale problems
        c = sc.random_problem(k)
        if int(c["prob"]["fix_scale"]):
            assert sc.solve(c, sc.DROP_SCALE)[0].tobytes() == sc.solve(c)[0].tobytes(), k


def test_a_finite_rejected_last_trial_leaves_the_same_errors(runs):
    """Why only z_zero shows a stale _error deciding a flag.  optimize() ends on a rejected trial only after ten rejections in a row
    (lambda has then grown by 2^55) or on rho == 0, or when rho is NaN.  With finite sums the rejected step is so small that the cached
    errors equal the fresh ones bit for bit: the largest |cached chi2 - fresh chi2| / th2 over all checks is exactly 0."""
    seen = 0
    for name, (c, r, st, info, mg) in runs.items():
        if c["exact"]:
            assert mg[sc.M_STALE] == 0.0 and info[sc.I_STALE_R1] == 0 and info[sc.I_STALE_R2] == 0, name
            seen += int(info[sc.I_LAST_REJECTED_R1] + info[sc.I_LAST_REJECTED_R2] > 0)
    assert seen >= 5
    assert runs["z_zero"][3][sc.I_STALE_R1] > 0


def test_shared_solver_and_quadratic_form_against_numpy():
    """sd_sim3_math.h also holds the LDL^T, the edge's quadratic form and the damping factor, which the oracle shares with the kernel:
    checked here against numpy, which shares nothing."""
    rng = np.random.default_rng(5)
    for trial in range(40):
        A = rng.normal(size=(9, 7)) * 10.0 ** rng.integers(-3, 4, 7)         # columns of very different size: the pivoting reorders
        H = A.T @ A
        if trial % 4 == 1:
            H[6, :] = 0; H[:, 6] = 0                                         # the fixed-scale system: lambda alone on the last diagonal
        b = rng.normal(size=7)
        lam = 1e-5 * np.abs(np.diag(H)).max()
        ok, x = sc.solve7(H, b, lam)
        ref = np.linalg.solve(H + lam * np.eye(7), b)
        assert ok and np.allclose(x, ref, rtol=1e-6 * np.linalg.cond(H + lam * np.eye(7)) ** 0.5, atol=0), trial
        assert np.linalg.norm((H + lam * np.eye(7)) @ x - b) <= 1e-9 * (np.linalg.norm(b) + np.linalg.norm(H) * np.linalg.norm(x)), trial
    x0 = np.arange(7.0)
    D = np.diag([3.0, 2.0, -1.0, 5.0, 1.0, 4.0, 6.0])
    Qm, _ = np.linalg.qr(rng.normal(size=(7, 7)))
    for H, positive in ((Qm @ D @ Qm.T, False), (-np.eye(7), False), (np.zeros((7, 7)), True), (Qm @ np.abs(D) @ Qm.T, True),
                        (Qm @ np.diag([3.0, 2.0, 0, 0, 1.0, 0, 6.0]) @ Qm.T, None)):
        ok, x = sc.solve7(H, np.ones(7), 0.0, x0)
        if positive is not None:
            assert ok == positive, H
        if not ok:
            assert np.array_equal(x, x0)                                     # x keeps its value: the caller applies the OLD update
    ok, x = sc.solve7(np.diag([1.0, 9.0, 4.0, 16.0, 25.0, 2.0, 3.0]), np.array([1.0, 9, 4, 16, 25, 2, 3]), 0.0)
    assert ok and np.array_equal(x, np.ones(7))                              # pure pivoting: the permutation is undone
    regions = set()
    for trial in range(20):
        e = rng.normal(size=2) * (0.5 if trial % 2 else 30.0); J = rng.normal(size=(2, 7)) * 100; w = float(rng.uniform(0.1, 1)); delta = 3.1622777
        H, b, rho0 = sc.accumulate(e, J, w, delta)
        chi = w * (e @ e)
        r0, r1 = (chi, 1.0) if chi <= delta * delta else (2 * np.sqrt(chi) * delta - delta * delta, delta / np.sqrt(chi))
        regions.add(bool(chi <= delta * delta))
        assert rho0 == pytest.approx(r0, rel=1e-13) and np.allclose(H, r1 * w * (J.T @ J), rtol=1e-12, atol=1e-9)
        assert np.allclose(b, -r1 * w * (J.T @ e), rtol=1e-12, atol=1e-9)
    assert regions == {True, False}                                          # both sides of the Huber kernel
    L = sc.oracle()
    for rho in (1e-9, 0.1, 0.5, 0.9, 1.0, 5.0):
        assert L.sd_sim3_opt_oracle_good_step_scale(rho) == pytest.approx(max(1 / 3, min(2 / 3, 1 - (2 * rho - 1) ** 3)), rel=1e-15)


def test_update_branches():
    est = np.array([0.1, -0.2, 0.05, 0.9, 0.3, -0.4, 2.0, 1.3]); est[:4] /= np.linalg.norm(est[:4])
    big_w, small_w = np.array([0.02, -0.03, 0.01]), np.array([2e-6, -3e-6, 1e-6])
    v = np.array([0.1, 0.2, -0.3])
    for w, sigma, branch in ((small_w, 2e-6, 0), (big_w, 2e-6, 1), (small_w, 0.05, 2), (big_w, 0.05, 3), (big_w, -0.05, 3)):
        out, br = sc.oplus(est, np.concatenate([w, v, [sigma]]), 0)
        assert br == branch
        # closed form in numpy: R = exp([w]x), s = e^sigma, t = W v with W integrated numerically
        th = np.linalg.norm(w); K = sc._skew(w)
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
        xs, wq = np.polynomial.legendre.leggauss(12)
        a = (xs + 1) / 2
        W = sum(0.5 * wi * np.exp(sigma * ai) * (np.eye(3) + np.sin(ai * th) / th * K + (1 - np.cos(ai * th)) / th ** 2 * (K @ K)) for ai, wi in zip(a, wq))
        s = np.exp(sigma)
        Re, te, se = sc.quat_to_R(est[:4]), est[4:7], est[7]
        assert np.allclose(sc.quat_to_R(out[:4]), R @ Re, atol=1e-9) and abs(out[7] - s * se) < 1e-12
        assert np.allclose(out[4:7], s * (R @ te) + W @ v, atol=1e-9)
        fixed, brf = sc.oplus(est, np.concatenate([w, v, [sigma]]), 1)          # _fix_scale: update[6] = 0 before Sim3(update)
        assert fixed[7] == est[7] and brf == (0 if th < 1e-5 else 1)


def test_chi2_decisions_keep_their_margin_and_the_record_is_reproduced(runs):
    with open(TOL_PATH) as f:
        tol = json.load(f)
    assert tol["chi2_margin_required"] == CHI2_MARGIN and tol["value_factor"] == 10 and tol["f32_ulps"] == 4
    assert set(tol["cases"]) == set(runs)
    noisy = 0
    for name, (c, r, st, info, mg) in runs.items():
        rec = tol["cases"][name]
        if c["exact"] and len(c["corr"]):
            assert mg[sc.M_CHI2] >= CHI2_MARGIN, (name, mg[sc.M_CHI2])
            assert rec["chi2_margin"] == pytest.approx(float(mg[sc.M_CHI2]), rel=1e-9), name
        sp = sc.spread(c, contracted=False)                     # the variants that depend on IEEE arithmetic alone: never above the record
        for f in sc.VALUE_FIELDS:
            if rec["spread"][f] is None:
                assert sp[f] != sp[f], (name, f)
            else:
                assert sp[f] <= rec["spread"][f], (name, f, sp[f], rec["spread"][f])
        noisy += rec["lm_counts_differ"]
    # what Q45 records: once a problem has converged the sign of rho is rounding noise, so iterations / trials / stop change with the
    # summation order in about half of the crafted cases -- no margin protects them, which is why the device is compared bit for bit
    # with the oracle in the kernel's own order.  The chi2 decisions (ret, n_bad, the state bytes) never change.
    assert noisy > 0
    # the LM margin: ten times the oracle's own flip distance (tools/sim3_opt_tolerance.py).  A case outside it keeps iterations /
    # trials / stop under every variant, the kernel's order included, and the GPU test holds it to the SEQUENTIAL oracle's counters
    assert tol["lm_margin"] == pytest.approx(10 * tol["lm_flip_distance"]) and 0 < tol["lm_margin"] < CHI2_MARGIN
    held = [n for n, v in tol["cases"].items() if v["lm_held"]]
    assert len(held) >= 12 and {"far_prior", "size_10", "size_65", "gate_19", "gate_20", "gate_21", "outliers_15_of_100"} <= set(held)
    for name, (c, r, st, info, mg) in runs.items():
        margin = sc.lm_margin_of(mg)
        assert bool(tol["cases"][name]["lm_held"]) == bool(c.get("sane", True) and margin >= tol["lm_margin"]), name
        for flags, contract in ((sc.REVERSE, "off"), (sc.WAVE, "off")) + (((0, "fast"),) if sc.have_fma() else ()):
            r2 = sc.solve(c, flags, contract)[0]
            if tol["cases"][name]["lm_held"]:
                assert sc.lm_counts(r2) == sc.lm_counts(r), (name, flags, contract)
            elif c.get("sane", True) and flags != sc.WAVE and sc.lm_counts(r2) != sc.lm_counts(r):
                assert margin <= tol["lm_flip_distance"], (name, margin)        # the recorded flip distance covers every flip seen
    for name, (c, r, st, info, mg) in runs.items():
        for flags, contract in ((sc.REVERSE, "off"), (sc.WAVE, "off")) + (((0, "fast"),) if sc.have_fma() else ()):
            r2, st2 = sc.solve(c, flags, contract)[:2]
            assert (r2["ret"], r2["n_bad"], r2["more_iterations"], r2["written"]) == (r["ret"], r["n_bad"], r["more_iterations"], r["written"]), name
            assert np.array_equal(st2, st), name


def test_private_sin_cos_exp_stay_within_one_ulp_of_the_library(tmp_path):
    exe = str(tmp_path / "sim3_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(sc.ROOT, "slam-dynamic_amd", "csrc"), "-o", exe,
                           os.path.join(sc.ROOT, "tests", "cpp", "sim3_math_check.cpp")])
    out = subprocess.run([exe, "400000"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr


def test_invalid_tables_are_refused_before_anything_is_launched(fe):
    c = sc.scene("ok", 12, 1)
    off, corr, probs = sc.pack([c])

    def code(*a):
        with pytest.raises(fe.SdError) as e:
            fe.sim3_optimize(*a)
        return e.value.code
    big = sc.scene("big", sc.MAX_N + 1, 1)
    assert code(*sc.pack([big])) == fe.SD_ERR_INVALID                                  # 4,097: never a truncation
    for th2 in (0.0, -1.0, np.nan):
        p = probs.copy(); p["th2"] = th2
        assert code(off, corr, p) == fe.SD_ERR_INVALID
    for field, k in (("R12", 4), ("t12", 1), ("s12", None)):
        for bad in (np.nan, np.inf):
            p = probs.copy()
            if k is None:
                p[field] = bad
            else:
                p[field][0, k] = bad
            assert code(off, corr, p) == fe.SD_ERR_INVALID
    assert code(off + 1, np.concatenate([corr[:1], corr]), probs) == fe.SD_ERR_INVALID   # offsets must start at 0
    two = sc.pack([c, c])
    dec = two[0].copy(); dec[1] = dec[2] + 1
    assert code(dec, two[1], two[2]) == fe.SD_ERR_INVALID                               # offsets must not decrease
    many = np.repeat(probs, sc.MAX_PROBLEMS + 1)
    assert code(np.zeros(len(many) + 1, np.int32), corr[:0], many) == fe.SD_ERR_INVALID
    assert fe.SIM3_OPT_CORR_DTYPE == sc.CORR_DTYPE and fe.SIM3_OPT_PROBLEM_DTYPE == sc.PROBLEM_DTYPE and fe.SIM3_OPT_RESULT_DTYPE == sc.RESULT_DTYPE


def test_fuzz_seeds_stay_within_the_skip_cap_on_the_oracle_alone():
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_sim3_opt", os.path.join(sc.ROOT, "tools", "fuzz_sim3_opt.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    n = 300
    cases, tables, seq, wave, skipped, spread, flips = fz.oracle_pass(n, CHI2_MARGIN)
    assert skipped.sum() <= fz.MAX_SKIPPED * n
    assert flips == 0                                          # no oracle variant changes ret or n_bad of any problem
    assert np.array_equal(seq[0]["ret"], wave[0]["ret"]) and np.array_equal(seq[1], wave[1])
    assert {bool(x) for x in seq[0]["ret"] >= 20} == {True, False} and {int(x) for x in seq[0]["more_iterations"]} == {5, 10}
    with open(os.path.join(sc.ROOT, "profiles", "sim3_opt_fuzz.json")) as f:
        rec = json.load(f)
    assert rec["problems"] == n and rec["skipped"] == int(skipped.sum()) and rec["skipped"] <= rec["max_skipped"] * n
