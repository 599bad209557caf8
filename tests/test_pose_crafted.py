"""The crafted PoseOptimization cases (tests/pose_crafted.py) on the CPU oracle: every case takes the path it exists for, meets what
its construction promises, and keeps its chi2 values away from the thresholds -- which is what lets test_gpu_pose_crafted.py demand
exact flags of the kernel.  Also: the table covers every branch the issue lists, and each of four deliberate breaks of the algorithm
changes the outcome of a named case."""
import numpy as np
import pytest

import pose_cases as pc
import pose_crafted as pcr


@pytest.mark.parametrize("name", pcr.names())
def test_case_takes_its_path_and_meets_its_expectation(name):
    c = pcr.cases()[name]
    res = pcr.oracle_result(name)
    r, T, flags, st, rep = res
    assert pcr.paths_missing(c, res) == [], rep
    ex = c["expect"]
    if ex is not None:
        assert np.array_equal(flags, ex["flags"]), np.nonzero(flags != ex["flags"])[0]
        assert r == ex["n_good"]
        if "T_bytes" in ex:
            assert T.tobytes() == ex["T_bytes"]
        if "T_close" in ex:
            assert pc.pose_close(T, ex["T_close"], 1e-5), np.abs(T - ex["T_close"]).max()
    if c["no_move"]:
        assert T.tobytes() == c["T0"].tobytes()
    assert r == len(flags) - int(flags.sum()) or len(flags) < 3
    if not c["on_threshold"]:
        assert rep["margin"] >= pcr.MARGIN, rep["margin"]


def test_path_report_changes_nothing():
    for name in ("exit_reentry", "probe_half_y", "depth_zero_mono", "size_9_noisy"):
        c = pcr.cases()[name]
        r, T, flags, st, _ = pcr.oracle_result(name)
        r2, T2, f2, st2 = pc.optimize(c["edges"], c["cam"], c["T0"])
        assert r == r2 and T.tobytes() == T2.tobytes() and np.array_equal(flags, f2) and np.array_equal(st, st2), name


def test_table_covers_every_listed_path():
    reps = {n: pcr.oracle_result(n)[4] for n in pcr.names()}
    want = {n: pcr.cases()[n]["paths"] for n in pcr.names()}
    # counted only where the case DECLARES the path, so the parametrised test above pins it
    quat = {p["quat"] for p in want.values() if "quat" in p}
    assert quat == set(pc.QUAT_BRANCHES)
    for b in ("i=0", "i=1", "i=2"):
        assert {p["w_flip"] for p in want.values() if p.get("quat") == b and "w_flip" in p} == {True, False}, b
    assert any("small_exp_min" in p for p in want.values())
    endings = {p[k] for p in want.values() for k in ("endings_all", "endings_any") if k in p}
    assert endings == set(pc.ROUND_ENDINGS[1:])
    assert any(p.get("reentered_min", 0) >= 1 for p in want.values())
    assert any(p.get("last_round_changes_min", 0) >= 1 for p in want.values())
    assert any(p.get("non_finite") for p in want.values())
    assert any(p.get("last_rejected") for p in want.values())
    # the quaternion of a step's exp takes the tr > 0 branch, except where the step is NaN (tr > 0 is false then)
    assert all(r["exp_quat"] == ["tr>0"] or r["non_finite"] for r in reps.values())
    sizes = {len(pcr.cases()[n]["edges"]) for n in pcr.names()}
    assert set(pcr.SIZES) <= sizes and max(sizes) == 513


def _differs(name, mode):
    """The oracle under a variant no longer gives what the case expects (its construction where it has one, else the reference run)."""
    c = pcr.cases()[name]
    r0, T0, f0, _, _ = pcr.oracle_result(name)
    r, T, f, _ = pc.optimize(c["edges"], c["cam"], c["T0"], mode)
    ex = c["expect"] or {}
    flags = ex.get("flags", f0)
    if r != ex.get("n_good", r0) or not np.array_equal(f, flags):
        return True
    if "T_bytes" in ex or c["no_move"]:
        return T.tobytes() != c["T0"].tobytes()
    return not pc.pose_close(T, ex.get("T_close", T0), 1e-5)


BREAKS = [  # (the break, the oracle option that makes it, a case whose expectation then fails)
    (">= in the classification", pc.MODE_GEQ, "probe_identity"),
    (">= in the classification", pc.MODE_GEQ, "probe_half_z"),
    ("classification compare in f64", pc.MODE_F64_COMPARE, "probe_half_x"),
    ("wrong sign of w in the i = 0 branch", pc.MODE_FLIP_BRANCH[0], "far_x_120p01_shifted"),
    ("wrong sign of w in the i = 1 branch", pc.MODE_FLIP_BRANCH[1], "far_y_120p01_shifted"),
    ("wrong sign of w in the i = 2 branch", pc.MODE_FLIP_BRANCH[2], "far_ztilt_119p99"),
    ("est where the classification reads errPose", pc.MODE_FRESH_ERRORS, "depth_zero_mono"),
]


@pytest.mark.parametrize("what,mode,name", BREAKS)
def test_a_deliberate_break_fails_a_named_case(what, mode, name):
    """The kernel is not run broken; the oracle under the same change stands in for it.  The GPU test compares the kernel with exactly
    these expectations, so a kernel with the break fails the same case."""
    assert not _differs(name, 0)
    assert _differs(name, mode), what


def test_f64_compare_and_geq_are_told_apart_by_different_probe_edges():
    """Probe pairs 0 (chi2 == 5.991f) and 2 (chi2 == 7.815f) flip under `>=` only; pair 4 (5.991f < chi2 < the next f32, rounded down to
    5.991f) flips under the f64 compare and, being equal to the threshold after the cast, under `>=` as well."""
    c = pcr.cases()["probe_identity"]
    base = c["expect"]["flags"]
    _, _, geq, _ = pc.optimize(c["edges"], c["cam"], c["T0"], pc.MODE_GEQ)
    _, _, f64, _ = pc.optimize(c["edges"], c["cam"], c["T0"], pc.MODE_F64_COMPARE)
    probe = np.arange(15, 25)
    assert np.nonzero(geq != base)[0].tolist() == [15, 16, 19, 20, 23, 24]
    assert np.nonzero(f64 != base)[0].tolist() == [23, 24]
    assert set(np.nonzero(base)[0]) <= set(probe)


def test_lambda_init_with_a_nan_diagonal_does_not_reach_the_output():
    """computeLambdaInit takes std::max(fabs(h), m), which keeps a NaN diagonal entry; the kernel's fmax skips it.  With a point on the
    camera plane H holds NaN off the diagonal whatever lambda is (J[0][4] = 0 times an infinite J[0][0]), every trial is rejected and
    the prior comes back: both rules give the same bytes."""
    for name in ("depth_zero_mono", "depth_zero_stereo"):
        c = pcr.cases()[name]
        a = pc.optimize(c["edges"], c["cam"], c["T0"])
        b = pc.optimize(c["edges"], c["cam"], c["T0"], pc.MODE_LAMBDA_FMAX)
        assert a[0] == b[0] == len(c["edges"]) and a[1].tobytes() == b[1].tobytes() == c["T0"].tobytes()
        assert not a[2].any() and not b[2].any() and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("k,N", list(enumerate(pcr.FRAME_SIZES)))
def test_uploaded_frame_problems_keep_the_margin_and_hold_the_pattern(k, N):
    """What test_gpu_pose_crafted.py uploads for k_pose_edges: the match pattern has the indices the ballot compaction can get wrong,
    and the pose problem its edges make keeps the margin."""
    f = pcr.edge_frames(N, 900 + k, pcr.inv_level_sigma2())
    m = f["match"]
    for i in (0, 63, 64, 255, 256, N - 1):
        assert i >= N or m[i] >= 0, i
    assert (m[96:160] >= 0).all() and (m[160:224] < 0).all() and m[0] == m[63]
    assert m.max() < N and len(f["edges"]) == (m >= 0).sum() and np.array_equal(f["edges"]["kp_index"], np.nonzero(m >= 0)[0])
    e = f["edges"]
    assert set(f["cur"]["kp"]["octave"][m >= 0]) == set(range(8)) and (e["ur"] < 0).any() and (e["ur"] == 0).any() and (e["ur"] > 0).any()
    r, T, flags, st, rep = pc.optimize_paths(e, f["cam"], f["T0"])
    assert rep["margin"] >= pcr.MARGIN and st[0] == 4 and 0 < flags.sum() < len(e)
