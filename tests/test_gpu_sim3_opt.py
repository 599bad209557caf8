"""k_sim3_optimize (sd_sim3_optimize_*) against the OptimizeSim3 CPU oracle on the crafted problems of tests/sim3_opt_cases.py.

Two comparisons (DESIGN Q45).  Against the oracle summing in the kernel's own fixed order, everything is equal bit for bit -- the
only way to hold iterations / trials / stop to equality, because once a problem has converged the sign of rho is rounding noise
(profiles/sim3_opt_tolerance.json: the LM counts of about half of the crafted cases change with the summation order of the oracle
alone).  Against the sequential oracle, the contract of DESIGN Q37: the chi2 decisions (ret, n_bad, more_iterations, written, every
state byte) are equal; iterations / trials / stop are equal on every case whose LM decisions lie outside ten times the oracle's own
flip distance (16 of 33); and q / t / s / T12 lie within max(10 x the oracle's own spread, 4 f32 ulps of the entry), the spread being
measured among the oracle as built, fed its edges in reverse and built with -ffp-contract=fast -- not in the kernel's order."""
import json
import os

import numpy as np
import pytest

import sim3_opt_cases as sc

pytestmark = pytest.mark.gpu
TOL_PATH = os.path.join(sc.ROOT, "profiles", "sim3_opt_tolerance.json")
F32_ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def cases():
    return sc.crafted_cases()


@pytest.fixture(scope="module")
def device_results(gpu, fe, cases):
    """All crafted cases in ONE call: (results, state, offsets)."""
    off, corr, probs = sc.pack(cases)
    res, st = fe.sim3_optimize(off, corr, probs)
    return res, st, off


def same_record(a, b):
    return all(np.array_equal(np.asarray(a[f]), np.asarray(b[f]), equal_nan=np.asarray(a[f]).dtype.kind == "f") for f in sc.RESULT_DTYPE.names)


def test_problem_ring_over_many_launches_on_two_streams(gpu, fe):
    """sd_sim3_optimize_device on the schedule of solver_ring.py (this solver has a ring and no workspace): every output byte of every
    call equals the problem run alone through the host form.  5 .. 50 correspondences: below and above the `< 10` return."""
    import ctypes as C
    import torch
    import solver_ring as sr
    pool = [sc.scene("ring_%d" % n, n, 50 + k, outliers=n // 8) for k, n in enumerate(range(5, 53, 3))]
    calls = sr.schedule(pool, lambda c: len(c["corr"]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def prepare(cs):
        off, corr, probs = sc.pack(cs)
        return dict(cs=cs, off=off, probs=probs, corr=torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda(),
                    res=torch.full((len(cs) * sc.RESULT_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda"),
                    st=torch.full((len(corr),), 0x5A, dtype=torch.uint8, device="cuda"))

    def enqueue(a, stream):
        fe.check(fe.lib().sd_sim3_optimize_device(len(a["cs"]), p(a["off"]), dp(a["corr"]), p(a["probs"]), dp(a["res"]), dp(a["st"]), C.c_void_p(stream)))

    done = sr.drive(calls, prepare, enqueue)
    alone = {}
    for k, a in enumerate(done):
        res = a["res"].cpu().numpy().view(sc.RESULT_DTYPE); st = a["st"].cpu().numpy(); off = a["off"]
        for q, c in enumerate(a["cs"]):
            if c["name"] not in alone:
                alone[c["name"]] = fe.sim3_optimize(*sc.pack([c]))
            r, s = alone[c["name"]]
            assert res[q].tobytes() == r[0].tobytes() and st[off[q]:off[q + 1]].tobytes() == s.tobytes(), (k, q, c["name"])


def test_every_crafted_problem_equals_the_oracle_in_the_kernels_order(device_results, cases):
    res, st, off = device_results
    for k, c in enumerate(cases):
        r, s = sc.solve(c, sc.WAVE)[:2]
        d = res[k]
        assert (d["ret"], d["n_bad"], d["more_iterations"], d["written"], d["n_correspondences"]) == \
               (r["ret"], r["n_bad"], r["more_iterations"], r["written"], r["n_correspondences"]), c["name"]
        assert d["iterations"].tolist() == r["iterations"].tolist() and d["trials"].tolist() == r["trials"].tolist() and \
               d["stop"].tolist() == r["stop"].tolist(), (c["name"], d, r)
        assert np.array_equal(st[off[k]:off[k + 1]], s), c["name"]
        assert same_record(d, r), (c["name"], d, r)


def test_contract_against_the_sequential_oracle(device_results, cases):
    res, st, off = device_results
    with open(TOL_PATH) as f:
        tol = json.load(f)
    held = 0
    for k, c in enumerate(cases):
        r, s = sc.solve(c)[:2]
        d = res[k]
        assert (d["ret"], d["n_bad"], d["more_iterations"], d["written"]) == (r["ret"], r["n_bad"], r["more_iterations"], r["written"]), c["name"]
        assert np.array_equal(st[off[k]:off[k + 1]], s), c["name"]
        if tol["cases"][c["name"]]["lm_held"]:                   # every LM decision outside ten times the oracle's own flip distance
            assert sc.lm_counts(d) == sc.lm_counts(r), (c["name"], sc.lm_counts(d), sc.lm_counts(r))
            held += 1
        for f in sc.VALUE_FIELDS:
            spread = tol["cases"][c["name"]]["spread"][f]
            a, b = np.asarray(d[f], np.float64), np.asarray(r[f], np.float64)
            if spread is None:
                assert np.array_equal(np.isnan(a), np.isnan(b)), (c["name"], f)
                continue
            bound = np.maximum(tol["value_factor"] * spread, tol["f32_ulps"] * F32_ULP * np.abs(b))
            assert (np.abs(a - b) <= bound).all(), (c["name"], f, np.abs(a - b).max(), spread)
    assert held >= 12


def test_a_problem_does_not_depend_on_its_neighbours_or_its_position(device_results, cases, fe):
    res, st, off = device_results
    pick = [k for k, c in enumerate(cases) if len(c["corr"]) <= 300]
    for k in pick:                                              # 1 problem per call
        r1, s1 = fe.sim3_optimize(*sc.pack([cases[k]]))
        assert r1[0].tobytes() == res[k].tobytes() and s1.tobytes() == st[off[k]:off[k + 1]].tobytes(), cases[k]["name"]
    a, b = pick[3], pick[-1]                                    # 2 problems per call, either way round
    r2, s2 = fe.sim3_optimize(*sc.pack([cases[b], cases[a]]))
    assert r2[0].tobytes() == res[b].tobytes() and r2[1].tobytes() == res[a].tobytes()
    order = [pick[(7 * i) % len(pick)] for i in range(65)]      # 65 problems per call, shuffled and repeated
    r65, s65 = fe.sim3_optimize(*sc.pack([cases[k] for k in order]))
    o65 = sc.pack([cases[k] for k in order])[0]
    for i, k in enumerate(order):
        assert r65[i].tobytes() == res[k].tobytes() and s65[o65[i]:o65[i + 1]].tobytes() == st[off[k]:off[k + 1]].tobytes(), (i, cases[k]["name"])


def test_host_and_device_forms_agree_and_repeat(device_results, cases, fe):
    res, st, off = device_results
    r, s = fe.sim3_optimize(*sc.pack(cases), device=True)
    assert r.tobytes() == res.tobytes() and s.tobytes() == st.tobytes()
    r, s = fe.sim3_optimize(*sc.pack(cases))
    assert r.tobytes() == res.tobytes() and s.tobytes() == st.tobytes()
    none, s0 = fe.sim3_optimize(np.zeros(1, np.int32), np.zeros(0, sc.CORR_DTYPE), np.zeros(0, sc.PROBLEM_DTYPE))
    assert len(none) == 0 and len(s0) == 0


def test_the_chain_gate_and_the_return_zero_path(device_results, cases):
    res, st, off = device_results
    by = {c["name"]: (res[k], st[off[k]:off[k + 1]], c) for k, c in enumerate(cases)}
    assert [int(by["gate_%d" % n][0]["ret"]) for n in (19, 20, 21)] == [19, 20, 21]
    for name in ("size_9", "far_prior_all_bad"):                # return 0: the prior comes back untouched, the NULLed matches stay
        d, s, c = by[name]
        assert d["ret"] == 0 and d["written"] == 0 and (s == 1).sum() == d["n_bad"]
        assert np.array_equal(d["t"], np.asarray(c["prob"]["t12"], np.float64)) and d["s"] == float(c["prob"]["s12"])
    assert by["far_prior_all_bad"][0]["n_bad"] == 59
    for fix in (0, 1):
        d, s, c = by["scale_2_fix%d" % fix]
        assert (d["s"] == 1.0) == bool(fix) and (fix or abs(d["s"] / 2.0 - 1) < 0.02)
    d, s, c = by["z_zero"]
    assert d["ret"] == 30 and d["n_bad"] == 0 and d["trials"].tolist() == [5, 5]   # NaN sums: every trial rejected, stale NaN errors flag nothing


def test_random_problems_in_one_call(gpu, fe):
    """The fuzz's first 130 problems in one call: bit for bit against the oracle in the kernel's order,
    the chi2 decisions equal to the sequential oracle's."""
    cases = [sc.random_problem(k) for k in range(130)]
    off, corr, probs = sc.pack(cases)
    res, st = fe.sim3_optimize(off, corr, probs)
    wave = sc.solve_packed(off, corr, probs, sc.WAVE, 16)
    seq = sc.solve_packed(off, corr, probs, 0, 16)
    for i in range(len(cases)):
        assert res[i].tobytes() == wave[0][i].tobytes(), (i, res[i], wave[0][i])
    assert st.tobytes() == wave[1].tobytes() == seq[1].tobytes()
    for f in ("ret", "n_bad", "more_iterations", "written"):
        assert np.array_equal(res[f], seq[0][f]), f
