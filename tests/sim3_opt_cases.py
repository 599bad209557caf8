"""Shared by test_sim3_opt_oracle.py, test_gpu_sim3_opt.py and tools/fuzz_sim3_opt.py: the OptimizeSim3 CPU oracle
(tests/cpp/sim3_opt_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory; it includes the kernel's own
slam-dynamic_amd/csrc/sd_sim3_math.h) and seeded crafted problems in plain numpy.

A case is dict(name, corr (CORR_DTYPE), prob (PROBLEM_DTYPE scalar), expect (dict of pinned facts), exact (bool: held to the margin
contract; False only for the cases whose sums are Inf / NaN)).  Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR_DTYPE = np.dtype([("xw1", "<f4", (3,)), ("xw2", "<f4", (3,)), ("obs1", "<f4", (2,)), ("obs2", "<f4", (2,)), ("inv_sigma2_1", "<f4"),
                       ("inv_sigma2_2", "<f4"), ("tag", "<i4")])                                              # sd_sim3_opt_corr
PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("R12", "<f4", (9,)),
                          ("t12", "<f4", (3,)), ("s12", "<f4"), ("th2", "<f4"), ("fix_scale", "<i4")])        # sd_sim3_opt_problem
RESULT_DTYPE = np.dtype([("ret", "<i4"), ("n_correspondences", "<i4"), ("n_bad", "<i4"), ("more_iterations", "<i4"),
                         ("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("stop", "<i4", (2,)), ("written", "<i4"), ("reserved", "<i4"),
                         ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("T12", "<f4", (16,))])        # sd_sim3_opt_result
assert CORR_DTYPE.itemsize == 52 and PROBLEM_DTYPE.itemsize == 220 and RESULT_DTYPE.itemsize == 176

K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)        # fx fy cx cy
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)   # mvInvLevelSigma2 of the default pyramid
MAX_N, MAX_PROBLEMS = 4096, 65535
STOP_OK, STOP_TRIALS, STOP_RHO_ZERO, STOP_NO_GAIN = 0, 1, 2, 3
# flags of the oracle: the deliberately wrong twins, and the reversed edge order
TWIN_ANALYTIC, TWIN_RECOMPUTE, TWIN_WRITE_ON_ZERO, TWIN_KEEP_LAMBDA, TWIN_SINGLE_CHI2, DROP_SCALE, REVERSE, WAVE = 1, 2, 4, 8, 16, 32, 64, 128
TWINS = {"analytic": TWIN_ANALYTIC, "recompute": TWIN_RECOMPUTE, "write_on_zero": TWIN_WRITE_ON_ZERO, "keep_lambda": TWIN_KEEP_LAMBDA,
         "single_chi2": TWIN_SINGLE_CHI2}
# info / margin slots of the oracle
I_BRANCH0, I_SOLVE_FAILED, I_REJECTED, I_LAST_REJECTED_R1, I_LAST_REJECTED_R2, I_STALE_R1, I_STALE_R2, I_NONFINITE, I_HUBER = 0, 4, 5, 6, 7, 8, 9, 10, 11
M_CHI2, M_RHO, M_STOP, M_STALE = 0, 1, 2, 3
N_INFO, N_MARGIN = 16, 4

_oracles = {}


def have_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read().replace("\n", " ")
    except OSError:
        return False


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast and FMA (for the spread)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="sim3_opt_oracle_")
        so = os.path.join(d, "libsim3_opt_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []              # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + [
            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "slam-dynamic_amd", "csrc"), "-shared", "-fPIC", "-o", so,
            os.path.join(ROOT, "tests", "cpp", "sim3_opt_oracle.cpp")])
        L = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        L.sd_sim3_opt_oracle.argtypes = [vp, vp, i, i, vp, vp, vp, vp]
        L.sd_sim3_opt_oracle_range.argtypes = [i, i, vp, vp, vp, i, vp, vp, vp, vp]
        L.sd_sim3_opt_oracle_jacobians.argtypes = [vp, vp, vp, vp, vp, vp]
        L.sd_sim3_opt_oracle_oplus.argtypes = [vp, vp, i, vp]
        L.sd_sim3_opt_oracle_oplus.restype = i
        L.sd_sim3_opt_oracle_objective.argtypes = [vp, vp, i, vp, vp]
        L.sd_sim3_opt_oracle_objective.restype = C.c_double
        L.sd_sim3_opt_oracle_solve7.argtypes = [vp, vp, C.c_double, vp]
        L.sd_sim3_opt_oracle_solve7.restype = i
        L.sd_sim3_opt_oracle_accumulate.argtypes = [C.c_double, C.c_double, vp, C.c_double, C.c_double, vp]
        L.sd_sim3_opt_oracle_good_step_scale.argtypes = [C.c_double]
        L.sd_sim3_opt_oracle_good_step_scale.restype = C.c_double
        _oracles[contract] = L
    return _oracles[contract]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def solve(case, flags=0, contract="off"):
    """OptimizeSim3 of one case on the CPU: (result (RESULT_DTYPE scalar), state (N,) u8, info (16,) int64, margins (4,) f64)."""
    c = np.ascontiguousarray(case["corr"], CORR_DTYPE)
    p = np.ascontiguousarray(case["prob"], PROBLEM_DTYPE).reshape(1)
    res = np.zeros(1, RESULT_DTYPE); st = np.zeros(max(len(c), 1), np.uint8); info = np.zeros(N_INFO, np.int64); mg = np.zeros(N_MARGIN)
    oracle(contract).sd_sim3_opt_oracle(_p(p), _p(c), len(c), flags, _p(res), _p(st), _p(info), _p(mg))
    return res[0], st[:len(c)], info, mg


def pack(cases):
    """(corr_offset, corr, problems) of a list of cases, as sd_sim3_optimize_* takes them."""
    off = np.zeros(len(cases) + 1, np.int32)
    off[1:] = np.cumsum([len(c["corr"]) for c in cases])
    corr = np.concatenate([np.ascontiguousarray(c["corr"], CORR_DTYPE) for c in cases]) if cases else np.zeros(0, CORR_DTYPE)
    probs = np.array([c["prob"] for c in cases], PROBLEM_DTYPE)
    return off, corr, probs


def jacobians(case, i, est):
    """(numeric J (4, 7), analytic J (4, 7), errors (4,)) of correspondence i's two edges at est = (qx qy qz qw t0 t1 t2 s)."""
    p = np.ascontiguousarray(case["prob"], PROBLEM_DTYPE).reshape(1)
    c = np.ascontiguousarray(case["corr"][i:i + 1], CORR_DTYPE)
    e = np.ascontiguousarray(est, np.float64)
    Jn = np.zeros((4, 7)); Ja = np.zeros((4, 7)); err = np.zeros(4)
    oracle().sd_sim3_opt_oracle_jacobians(_p(p), _p(c), _p(e), _p(Jn), _p(Ja), _p(err))
    return Jn, Ja, err


def objective(case, est, live):
    """The oracle's activeRobustChi2 at est over the correspondences with live[i] set."""
    c = np.ascontiguousarray(case["corr"], CORR_DTYPE); p = np.ascontiguousarray(case["prob"], PROBLEM_DTYPE).reshape(1)
    lv = np.ascontiguousarray(live, np.uint8); e = np.ascontiguousarray(est, np.float64)
    return float(oracle().sd_sim3_opt_oracle_objective(_p(p), _p(c), len(c), _p(lv), _p(e)))


def solve7(H, b, lam, x0=None):
    """(isPositive(), x) of the shared pivoted LDL^T on the symmetric 7 x 7 H (its lower triangle is passed) plus lam * I."""
    H = np.asarray(H, np.float64)
    low = np.ascontiguousarray([H[i, j] for i in range(7) for j in range(i + 1)], np.float64)
    x = np.zeros(7) if x0 is None else np.array(x0, np.float64)
    bb = np.ascontiguousarray(b, np.float64)
    ok = oracle().sd_sim3_opt_oracle_solve7(_p(low), _p(bb), float(lam), _p(x))
    return bool(ok), x


def accumulate(e, J, w, delta):
    """One edge's share of the system: (H (7, 7) lower triangle filled symmetric, b (7,), rho0)."""
    v = np.zeros(36); JJ = np.ascontiguousarray(J, np.float64)
    oracle().sd_sim3_opt_oracle_accumulate(float(e[0]), float(e[1]), _p(JJ), float(w), float(delta), _p(v))
    H = np.zeros((7, 7)); k = 0
    for i in range(7):
        for j in range(i + 1):
            H[i, j] = H[j, i] = v[k]; k += 1
    return H, v[28:35].copy(), float(v[35])


def oplus(est, update, fix_scale):
    """(Sim3(update) * est as 8 doubles, the branch of Sim3(update))."""
    e = np.ascontiguousarray(est, np.float64); u = np.ascontiguousarray(update, np.float64); out = np.zeros(8)
    br = oracle().sd_sim3_opt_oracle_oplus(_p(e), _p(u), int(fix_scale), _p(out))
    return out, br


# ---------------------------------------------------------------- plain numpy f64 restatement (checks the oracle, shares no code with it)
def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def camera_points(case):
    """(X1c, X2c) (N, 3) f64: the f32 camera coordinates the fixed point vertices hold."""
    p, c = case["prob"], case["corr"]
    out = []
    for T, xw in ((p["Tcw1"], c["xw1"]), (p["Tcw2"], c["xw2"])):
        T = np.asarray(T, np.float32).reshape(4, 4)
        cols = []
        for r in range(3):
            s = (T[r, 0] * xw[:, 0] + T[r, 1] * xw[:, 1]).astype(np.float32)
            s = (s + T[r, 2] * xw[:, 2]).astype(np.float32)
            cols.append((s + T[r, 3]).astype(np.float32))
        out.append(np.stack(cols, 1).astype(np.float64))
    return out


def np_errors(case, est):
    """The four residuals of every correspondence at est: (N, 4)."""
    X1, X2 = camera_points(case)
    p, c = case["prob"], case["corr"]
    R, t, s = quat_to_R(est[:4]), np.asarray(est[4:7]), est[7]
    K1, K2 = np.asarray(p["K1"], np.float64), np.asarray(p["K2"], np.float64)
    P = (s * (R @ X2.T)).T + t
    Q = ((R.T @ (X1 - t).T) / s).T
    with np.errstate(all="ignore"):
        e12 = c["obs1"].astype(np.float64) - np.stack([P[:, 0] / P[:, 2] * K1[0] + K1[2], P[:, 1] / P[:, 2] * K1[1] + K1[3]], 1)
        e21 = c["obs2"].astype(np.float64) - np.stack([Q[:, 0] / Q[:, 2] * K2[0] + K2[2], Q[:, 1] / Q[:, 2] * K2[1] + K2[3]], 1)
    return np.concatenate([e12, e21], 1)


def np_objective(case, est, live=None):
    """The active robust chi2 at est over the live correspondences."""
    e = np_errors(case, est)
    c, th2 = case["corr"], float(case["prob"]["th2"])
    delta = float(np.float32(np.sqrt(np.float32(th2))))
    w1, w2 = c["inv_sigma2_1"].astype(np.float64), c["inv_sigma2_2"].astype(np.float64)
    with np.errstate(all="ignore"):                  # error . (information * error) with the dense 2 x 2 information: 0 * Inf is NaN there
        chi = np.concatenate([e[:, 0] * (w1 * e[:, 0] + 0.0 * e[:, 1]) + e[:, 1] * (0.0 * e[:, 0] + w1 * e[:, 1]),
                              e[:, 2] * (w2 * e[:, 2] + 0.0 * e[:, 3]) + e[:, 3] * (0.0 * e[:, 2] + w2 * e[:, 3])])
    if live is not None:
        chi = chi[np.concatenate([live, live])]
    with np.errstate(all="ignore"):
        rho = np.where(chi <= delta * delta, chi, 2 * np.sqrt(chi) * delta - delta * delta)
    return float(rho.sum())


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def np_analytic_jacobian(case, i, est):
    """d(residuals) / d(update) of correspondence i for estimate <- Sim3(update) * estimate, (4, 7): columns omega, upsilon, sigma."""
    X1, X2 = camera_points(case)
    p = case["prob"]
    R, t, s = quat_to_R(est[:4]), np.asarray(est[4:7]), est[7]
    K1, K2 = np.asarray(p["K1"], np.float64), np.asarray(p["K2"], np.float64)
    J = np.zeros((4, 7))
    P = s * (R @ X2[i]) + t
    dP = np.concatenate([-_skew(P), np.eye(3), P[:, None]], 1)
    Q = R.T @ (X1[i] - t) / s
    dQ = (R.T / s) @ np.concatenate([_skew(X1[i]), -np.eye(3), -X1[i][:, None]], 1)
    for row, (Y, dY, K) in enumerate(((P, dP, K1), (Q, dQ, K2))):
        J[2 * row] = -K[0] * (dY[0] / Y[2] - Y[0] / Y[2] ** 2 * dY[2])
        J[2 * row + 1] = -K[1] * (dY[1] / Y[2] - Y[1] / Y[2] ** 2 * dY[2])
    if int(p["fix_scale"]):
        J[:, 6] = 0
    return J


# ---------------------------------------------------------------- scenes
def rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = _skew(a)
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def scene(name, N, seed, s=1.0, fix=0, noise=0.5, outliers=0, outlier_px=40.0, prior=(0.02, 0.1, 0.03), th2=10.0, K1=K_KITTI, K2=K_TUM,
          octaves=None, identity_poses=False, outliers2=0, behind=0, expect=None, exact=True):
    """N correspondences of two key frames whose camera frames are related by X1c = s R X2c + t; `noise` px of Gaussian noise on
    both observations, `outliers` correspondences (a seeded choice) moved by `outlier_px` in KF1's image and `outliers2` others in
    KF2's, the first `behind` points placed behind KF1's camera (consistently: no edge has a depth test), the prior off by a
    rotation of prior[0] rad, a translation of prior[1] and a log-scale of prior[2] (0 when the scale is fixed)."""
    rng = np.random.default_rng([seed, N, 7])
    R12 = rot(rng.normal(size=3), 0.3); t12 = rng.normal(size=3) * 0.5
    if fix:
        s = 1.0
    T1 = np.eye(4) if identity_poses else pose(rot(rng.normal(size=3), 0.4), rng.normal(size=3))
    T2 = np.eye(4) if identity_poses else pose(rot(rng.normal(size=3), 0.7), rng.normal(size=3) * 2)
    T1f, T2f = T1.astype(np.float32), T2.astype(np.float32)
    z = rng.uniform(4, 20, N)
    z[:behind] = -z[:behind]
    u = rng.uniform(100, 1100, N); v = rng.uniform(40, 330, N)
    X1c = np.stack([(u - K1[2]) / K1[0] * z, (v - K1[3]) / K1[1] * z, z], 1)
    X2c = ((R12.T @ (X1c - t12).T) / s).T
    c = np.zeros(N, CORR_DTYPE)
    c["xw1"] = ((X1c - T1[:3, 3]) @ T1[:3, :3]).astype(np.float32)
    c["xw2"] = ((X2c - T2[:3, 3]) @ T2[:3, :3]).astype(np.float32)
    o1 = np.stack([X1c[:, 0] / X1c[:, 2] * K1[0] + K1[2], X1c[:, 1] / X1c[:, 2] * K1[1] + K1[3]], 1)
    o2 = np.stack([X2c[:, 0] / X2c[:, 2] * K2[0] + K2[2], X2c[:, 1] / X2c[:, 2] * K2[1] + K2[3]], 1)
    o1 = o1 + rng.normal(size=(N, 2)) * noise; o2 = o2 + rng.normal(size=(N, 2)) * noise
    bad = np.zeros(N, bool)
    if outliers or outliers2:
        perm = rng.permutation(N)
        ang = rng.uniform(0, 2 * np.pi, N)
        off = outlier_px * np.stack([np.cos(ang), np.sin(ang)], 1)
        o1[perm[:outliers]] += off[perm[:outliers]]
        o2[perm[outliers:outliers + outliers2]] += off[perm[outliers:outliers + outliers2]]
        bad[perm[:outliers + outliers2]] = True
    c["obs1"] = o1.astype(np.float32); c["obs2"] = o2.astype(np.float32)
    oc = rng.integers(0, 8, (N, 2)) if octaves is None else np.broadcast_to(np.asarray(octaves), (N, 2))
    c["inv_sigma2_1"] = INV_SIGMA2[oc[:, 0]]; c["inv_sigma2_2"] = INV_SIGMA2[oc[:, 1]]
    c["tag"] = np.sort(rng.choice(max(2 * N, 1), N, replace=False)) if N else 0
    p = np.zeros((), PROBLEM_DTYPE)
    p["Tcw1"] = T1f.reshape(-1); p["Tcw2"] = T2f.reshape(-1); p["K1"] = K1; p["K2"] = K2
    Rp = rot(rng.normal(size=3), prior[0]) @ R12 if prior[0] else R12
    p["R12"] = Rp.astype(np.float32).reshape(-1)
    p["t12"] = (t12 + rng.normal(size=3) * prior[1]).astype(np.float32)
    p["s12"] = np.float32(s * (1.0 if fix else np.exp(prior[2])))
    p["th2"] = th2; p["fix_scale"] = fix
    return dict(name=name, corr=c, prob=p, bad=bad, truth=(s, R12, t12), expect=expect or {}, exact=exact)


def from_result(case, r, name, expect=None):
    """The same correspondences with the prior replaced by a result's estimate (rounded to the f32 the ABI takes)."""
    out = dict(case, name=name, expect=expect or {})
    p = case["prob"].copy()
    p["R12"] = quat_to_R(np.asarray(r["q"])).astype(np.float32).reshape(-1); p["t12"] = np.asarray(r["t"], np.float32); p["s12"] = np.float32(r["s"])
    out["prob"] = p
    return out


def z_zero_case():
    """Two points whose S12.map() has z == 0 exactly at the prior (identity rotation, unit scale, t12.z = 0, X2c.z = 0): their errors are
    Inf / NaN, the sums NaN, every trial is rejected (rho is NaN) and the restored estimate is the prior; chi2() then reads the NaN
    errors of the rejected trial, NaN > th2 is false and nothing is flagged -- although the prior is far enough off that fresh errors
    would flag most correspondences.  The stale _error decides every flag."""
    c = scene("z_zero", 30, 36, identity_poses=True, prior=(0.05, 0.3, 0), exact=False)
    c["prob"]["R12"] = np.eye(3, dtype=np.float32).reshape(-1); c["prob"]["t12"] = (0.5, 0.2, 0); c["prob"]["s12"] = 1
    c["corr"]["xw2"][4] = (1, 2, 0); c["corr"]["xw2"][5] = (0, 0, 0)
    return c


def crafted_cases():
    """Every crafted case, in a fixed order.  `expect` pins what the sequential arithmetic reaches (test_sim3_opt_oracle.py)."""
    out = []
    for N in (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, MAX_N):          # around the < 10 return, the wave and four waves, the cap
        out.append(scene("size_%d" % N, N, 1, expect=dict(ret=N if N >= 10 else 0, n_bad=0, more=5, written=int(N >= 10))))
    out.append(scene("outliers_15_of_100", 100, 2, outliers=15, expect=dict(ret=85, n_bad=15, more=10)))
    out.append(scene("outliers_in_kf2_only", 100, 4, outliers2=12, expect=dict(ret=88, n_bad=12, more=10)))
    for k in (6, 5, 4):                                                     # the chain's gate: ret >= 20
        out.append(scene("gate_%d" % (25 - k), 25, 11, outliers=k, expect=dict(ret=25 - k, n_bad=k, more=10)))
    for fix in (0, 1):
        for s in (0.5, 2.0):
            out.append(scene("scale_%g_fix%d" % (s, fix), 80, 3, s=s, fix=fix, expect=dict(ret=80, n_bad=0, fix=fix)))
    out.append(scene("far_prior_all_bad", 60, 29, prior=(0.6, 2.0, 0.5), outliers=6, expect=dict(ret=0, n_bad=59, more=10, written=0)))
    out.append(scene("far_prior", 60, 20, prior=(0.6, 2.0, 0.5), outliers=6, expect=dict(ret=54, n_bad=6, more=10)))
    c = scene("converged", 60, 35, noise=1.0)
    r = solve(c)[0]
    out.append(from_result(c, r, "start_at_optimum", expect=dict(ret=60, stop0=STOP_NO_GAIN, iterations0=3)))
    out.append(scene("exact_prior_noise_free", 40, 33, noise=0.0, prior=(0, 0, 0), expect=dict(ret=40, branch=0)))
    out.append(scene("scale_only_prior", 40, 34, noise=0.0, prior=(0, 0, 0.2), expect=dict(ret=40, branch=2)))
    c = scene("one_point_repeated", 30, 31, expect=dict(solve_failed=0))    # rank 4: lambda I keeps the matrix positive, isPositive() holds
    c["corr"][:] = c["corr"][0]
    out.append(c)
    c = scene("points_on_a_line", 30, 38, expect=dict(solve_failed=0))
    t = np.linspace(0.0, 1.0, 30, dtype=np.float32)[:, None]
    c["corr"]["xw1"] = c["corr"]["xw1"][0] + t * (c["corr"]["xw1"][1] - c["corr"]["xw1"][0])
    c["corr"]["xw2"] = c["corr"]["xw2"][0] + t * (c["corr"]["xw2"][1] - c["corr"]["xw2"][0])
    out.append(c)
    c = scene("negative_information", 30, 32, expect=dict(solve_failed=1))  # the one input that makes H indefinite: tempChi = DBL_MAX
    c["corr"]["inv_sigma2_1"] = -1; c["corr"]["inv_sigma2_2"] = -1
    c["sane"] = False                                                       # an indefinite system has no minimum: outside the LM margin rule
    out.append(c)
    out.append(z_zero_case())
    out.append(scene("behind_camera", 30, 37, behind=3, expect=dict(ret=30, n_bad=0)))
    out.append(scene("octaves_0_and_7", 50, 39, octaves=(0, 7), expect=dict(ret=50)))
    out.append(scene("octaves_7_and_0", 50, 39, octaves=(7, 0), expect=dict(ret=50)))
    return out


VALUE_FIELDS = ("q", "t", "s", "T12")


def variants(case, contracted=True):
    """The oracle's own variants, as the issue defines the spread: fed the edges in reverse and (contracted, where the host has FMA)
    built with -ffp-contract=fast.  The kernel's summation order is NOT among them: what the device is held to must not feed its bound."""
    return [solve(case, REVERSE)] + ([solve(case, 0, "fast")] if contracted and have_fma() else [])


def lm_counts(r):
    return (r["iterations"].tolist(), r["trials"].tolist(), r["stop"].tolist())


def lm_margin_of(mg):
    """The smallest relative distance of an LM decision (the sign of rho, the stop rule) from its threshold."""
    return float(min(mg[M_RHO], mg[M_STOP]))


def spread(case, contracted=True):
    """The largest difference per value field between the oracle as built and its variants(); plus whether a variant changes the LM
    counters.  NaN where a value is NaN."""
    base = solve(case)[0]
    runs = [v[0] for v in variants(case, contracted)]
    out = {}
    for f in VALUE_FIELDS:
        with np.errstate(invalid="ignore"):
            d = [np.abs(np.asarray(r[f], np.float64) - np.asarray(base[f], np.float64)).max() for r in runs]
        out[f] = float(np.max(d))
    out["lm_counts_differ"] = int(any(lm_counts(r) != lm_counts(base) for r in runs))
    return out


def solve_packed(off, corr, probs, flags=0, threads=1, contract="off"):
    """solve() of every problem of packed tables: -> (results (n,), state (E,), info (n, 16), margins (n, 4)).  Each of `threads` host
    threads makes ONE call that loops over a contiguous chunk of problems in C (ctypes drops the interpreter lock for it)."""
    from concurrent.futures import ThreadPoolExecutor
    n = len(off) - 1
    off = np.ascontiguousarray(off, np.int32); corr = np.ascontiguousarray(corr, CORR_DTYPE); probs = np.ascontiguousarray(probs, PROBLEM_DTYPE)
    res = np.zeros(max(n, 1), RESULT_DTYPE); st = np.zeros(max(len(corr), 1), np.uint8)
    info = np.zeros((max(n, 1), N_INFO), np.int64); mg = np.zeros((max(n, 1), N_MARGIN))
    L = oracle(contract)
    cuts = np.linspace(0, n, max(1, min(threads, n)) + 1).astype(int)

    def run(k):
        L.sd_sim3_opt_oracle_range(int(cuts[k]), int(cuts[k + 1]), _p(off), _p(corr), _p(probs), flags, _p(res), _p(st), _p(info), _p(mg))
    if len(cuts) == 2:
        run(0)
    else:
        with ThreadPoolExecutor(len(cuts) - 1) as pool:
            list(pool.map(run, range(len(cuts) - 1)))
    return res[:n], st[:len(corr)], info[:n], mg[:n]


def random_problem(seed):
    """A seeded problem of the fuzz and the benchmark: 20 - 300 correspondences, up to 30 % outliers in either image, either scale mode."""
    rng = np.random.default_rng([seed, 99])
    N = int(rng.integers(20, 301))
    return scene("fuzz_%d" % seed, N, 1000 + seed, s=float(rng.choice([0.7, 1.0, 1.4])), fix=int(rng.integers(0, 2)), noise=float(rng.uniform(0.2, 1.2)),
                 outliers=int(N * rng.uniform(0, 0.2)), outliers2=int(N * rng.uniform(0, 0.1)),
                 prior=(float(rng.uniform(0, 0.05)), float(rng.uniform(0, 0.3)), float(rng.uniform(0, 0.1))))
