"""TEST INFRASTRUCTURE shared by tests/test_pnp_oracle.py, tests/test_gpu_pnp.py and tools/fuzz_pnp.py: the ctypes binding of the PnPsolver
CPU oracle (tests/cpp/pnp_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory), seeded crafted problems in
the records of sd_pnp_ransac_*, and a numpy / float64 restatement of EPnP."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR_DTYPE = np.dtype([("xw", "<f4", (3,)), ("uv", "<f4", (2,)), ("sigma2", "<f4"), ("tag", "<i4")])                    # sd_pnp_corr
PROBLEM_DTYPE = np.dtype([("K", "<f4", (4,)), ("seed", "<u8"), ("start_iteration", "<i4"), ("n_iterations", "<i4")])    # sd_pnp_problem
RESULT_DTYPE = np.dtype([("kind", "<i4"), ("no_more", "<i4"), ("iteration", "<i4"), ("n_inliers", "<i4"), ("best_iteration", "<i4"),
                         ("best_inliers", "<i4"), ("n_refines", "<i4"), ("min_inliers", "<i4"), ("max_its", "<i4"), ("reserved", "<i4"),
                         ("Tcw", "<f4", (16,))])                                                                         # sd_pnp_result
MAX_N, MAX_ITS, CHUNK = 4096, 4096, 1024
K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)        # fx fy cx cy
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
DEFAULTS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)     # Tracking.cc:2266
TWINS = {"none": 0, "refine_ge": 1, "best_ge": 2, "refine_current": 3, "loop_and": 4, "err_le": 5, "pow4": 6}
INFO = ("kind", "iterations", "refine_calls", "best_updates", "ties", "hyp_flags", "win1", "win2", "win3", "refine_flags", "refine_winner",
        "refine_fails", "distinct_refines", "below_min")
F_B4_NEG, F_B4_ZERO, F_B3_1_NEG, F_SIGN, F_DET = 1, 2, 4, 8, 16
SIGMA2 = (1.2 ** np.arange(8, dtype=np.float32)) ** 2                         # mvLevelSigma2 of the default pyramid, f32

_oracles = {}


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast and FMA (to measure the spread)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="pnp_oracle_")
        so = os.path.join(d, "libpnp_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []              # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "pnp_oracle.cpp")])
        L = C.CDLL(so)
        vp, i, f, d_ = C.c_void_p, C.c_int, C.c_float, C.c_double
        L.sd_pnp_oracle_iterate.argtypes = [vp, vp, i, d_, i, i, i, f, f, i, i, vp, vp, vp]
        L.sd_pnp_oracle_iterate_range.argtypes = [i, i, vp, vp, vp, d_, i, i, i, f, f, i, vp, vp, vp]
        L.sd_pnp_oracle_hypotheses.argtypes = [vp, vp, i, f, i, vp, vp, vp]
        L.sd_pnp_oracle_sample.argtypes = [C.c_uint64, i, i, vp]
        L.sd_pnp_oracle_sample_closed.argtypes = [C.c_uint64, i, i, vp]
        L.sd_pnp_oracle_pose.argtypes = [vp, i, vp, i, vp, vp]
        L.sd_pnp_oracle_check.argtypes = [vp, vp, i, vp, vp]
        L.sd_pnp_oracle_refine.argtypes = [vp, i, vp, vp, i, vp, vp]
        L.sd_pnp_oracle_params.argtypes = [d_, i, i, i, f, i, i, vp]
        L.sd_pnp_oracle_svd.argtypes = [vp, i, i, vp, vp, vp]
        assert L.sd_pnp_oracle_info_count() == len(INFO)
        _oracles[contract] = L
    return _oracles[contract]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def params_of(pr):
    return {k: pr.get(k, v) for k, v in DEFAULTS.items()}


def _args(pr):
    a = params_of(pr)
    return (float(a["probability"]), int(a["min_inliers"]), int(a["max_iterations"]), int(a["min_set"]), float(a["epsilon"]), float(a["th2"]))


def iterate(pr, order=0, twin="none", contract="off"):
    """PnPsolver::iterate of one problem on the CPU: (result (RESULT_DTYPE scalar), inliers (N,) u8, info {name: int})."""
    c = np.ascontiguousarray(pr["corr"], CORR_DTYPE)
    p = np.ascontiguousarray(pr["prob"], PROBLEM_DTYPE).reshape(1)
    res = np.zeros(1, RESULT_DTYPE); inl = np.zeros(max(len(c), 1), np.uint8); info = np.zeros(len(INFO), np.int64)
    oracle(contract).sd_pnp_oracle_iterate(_p(p), _p(c), len(c), *_args(pr), int(order), TWINS[twin], _p(res), _p(inl), _p(info))
    return res[0], inl[:len(c)], dict(zip(INFO, (int(v) for v in info)))


def iterate_packed(off, corr, probs, args, order=0, threads=1):
    """iterate() of every problem of packed tables (pack()) -> (results (n,), inliers (E,)); `threads` host threads, one C call each."""
    from concurrent.futures import ThreadPoolExecutor
    n = len(probs)
    res = np.zeros(max(n, 1), RESULT_DTYPE); inl = np.zeros(max(len(corr), 1), np.uint8)
    L = oracle()
    a = (_p(off), _p(corr), _p(probs), float(args["probability"]), int(args["min_inliers"]), int(args["max_iterations"]), int(args["min_set"]),
         float(args["epsilon"]), float(args["th2"]), int(order), _p(res), _p(inl), None)
    cuts = [n * k // threads for k in range(threads + 1)]
    run = lambda k: L.sd_pnp_oracle_iterate_range(cuts[k], cuts[k + 1], *a)
    if threads == 1:
        run(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(run, range(threads)))
    return res[:n], inl[:len(corr)]


def end_of(pr, res):
    """The last iteration a call evaluates: max(max_its, start + n_iterations), 0 when N < min_inliers."""
    if len(pr["corr"]) < res["min_inliers"]:
        return 0
    p = np.ascontiguousarray(pr["prob"], PROBLEM_DTYPE).reshape(1)[0]
    return max(int(res["max_its"]), int(p["start_iteration"]) + int(p["n_iterations"]))


def hypotheses(pr, n_its, contract="off"):
    """(counts (n_its,), poses (n_its, 12) f64 [mRi | mti], masks (n_its, N)) of iterations 1 .. n_its, each evaluated as the loop would."""
    c = np.ascontiguousarray(pr["corr"], CORR_DTYPE)
    p = np.ascontiguousarray(pr["prob"], PROBLEM_DTYPE).reshape(1)
    cnt = np.zeros(max(n_its, 1), np.int32); poses = np.zeros((max(n_its, 1), 12)); masks = np.zeros((max(n_its, 1), max(len(c), 1)), np.uint8)
    masks = np.zeros((max(n_its, 1), len(c)), np.uint8) if len(c) else masks
    oracle(contract).sd_pnp_oracle_hypotheses(_p(p), _p(c), len(c), float(params_of(pr)["th2"]), int(n_its), _p(cnt), _p(poses), _p(masks))
    return cnt[:n_its], poses[:n_its], masks[:n_its]


def rows_of(pr):
    """(N, 6) f32 rows x y z u v maxError, the layout the oracle's stage exports take."""
    c = np.ascontiguousarray(pr["corr"], CORR_DTYPE)
    r = np.zeros((len(c), 6), np.float32)
    r[:, :3] = c["xw"]; r[:, 3:5] = c["uv"]; r[:, 5] = c["sigma2"] * np.float32(params_of(pr)["th2"])
    return r


def pose(rows, K, order=0, contract="off"):
    """compute_pose on given rows -> (R (3, 3), t (3,), extra dict)."""
    rows = np.ascontiguousarray(rows, np.float32)
    cam = np.asarray(K, np.float64).copy(); out = np.zeros(12); extra = np.zeros(17)
    oracle(contract).sd_pnp_oracle_pose(_p(rows), len(rows), _p(cam), int(order), _p(out), _p(extra))
    return out[:9].reshape(3, 3), out[9:], dict(winner=int(extra[0]), flags=int(extra[1]), rep=extra[2:5].copy(), w12=extra[5:17].copy())


def check(pose12, rows, K, contract="off"):
    rows = np.ascontiguousarray(rows, np.float32)
    cam = np.asarray(K, np.float64).copy(); mask = np.zeros(max(len(rows), 1), np.uint8)
    n = oracle(contract).sd_pnp_oracle_check(_p(np.ascontiguousarray(pose12, np.float64)), _p(rows), len(rows), _p(cam), _p(mask))
    return n, mask[:len(rows)]


def refine(rows, mask, K, order=0, contract="off"):
    rows = np.ascontiguousarray(rows, np.float32); mask = np.ascontiguousarray(mask, np.uint8)
    cam = np.asarray(K, np.float64).copy(); out = np.zeros(12); ref = np.zeros(max(len(rows), 1), np.uint8)
    n = oracle(contract).sd_pnp_oracle_refine(_p(rows), len(rows), _p(mask), _p(cam), int(order), _p(out), _p(ref))
    return n, out, ref[:len(rows)]


def ransac_parameters(N, twin="none", **kw):
    a = dict(DEFAULTS, **kw); out = np.zeros(2, np.int32)
    oracle().sd_pnp_oracle_params(float(a["probability"]), int(a["min_inliers"]), int(a["max_iterations"]), int(a["min_set"]), float(a["epsilon"]),
                                  int(N), TWINS[twin], _p(out))
    return int(out[0]), int(out[1])


def svd(A):
    A = np.ascontiguousarray(A, np.float64); m, n = A.shape
    w = np.zeros(n); U = np.zeros((m, n)); V = np.zeros((n, n))
    oracle().sd_pnp_oracle_svd(_p(A), m, n, _p(w), _p(U), _p(V))
    return U, w, V


def sample_literal(seed, it, N):
    out = np.zeros(4, np.int32); oracle().sd_pnp_oracle_sample(int(seed), int(it), int(N), _p(out)); return out


def sample_closed(seed, it, N):
    out = np.zeros(4, np.int32); oracle().sd_pnp_oracle_sample_closed(int(seed), int(it), int(N), _p(out)); return out


# ---- geometry ----
def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(R, t, X, K):
    Xc = X @ R.T + t
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1), Xc


def make_problem(seed, N, outliers=0.0, noise=0.0, K=K_KITTI, depth=(4.0, 30.0), planar=0.0, start=0, n_iterations=5, octaves=True, name=None,
                 **params):
    """A seeded scene: N world points in front of a camera at a random pose, their images (+ gaussian `noise` px), a fraction `outliers` of
    the images replaced by uniform ones.  planar > 0 squeezes the points onto a plane to that relative thickness.  Returns a dict with
    corr, prob, the SetRansacParameters arguments, the true pose (R, t) and `bad` (the outlier rows)."""
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.normal(size=3) * 0.3); t = rng.normal(size=3) * 0.5
    z = rng.uniform(depth[0], depth[1], N)
    if planar > 0:
        z = depth[0] + (depth[1] - depth[0]) * (0.5 + planar * (rng.uniform(size=N) - 0.5))
    W, H = 2 * float(K[2]), 2 * float(K[3])
    uv = np.stack([rng.uniform(0.05 * W, 0.95 * W, N), rng.uniform(0.05 * H, 0.95 * H, N)], 1)
    Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], 1)
    Xw = ((Xc - t) @ R).astype(np.float32)                            # R^T (Xc - t)
    uv, _ = project(R, t, Xw.astype(np.float64), K.astype(np.float64))
    uv = uv + rng.normal(size=uv.shape) * noise
    bad = np.zeros(N, bool)
    nb = int(round(outliers * N))
    if nb:
        bad[rng.permutation(N)[:nb]] = True
        uv[bad] = np.stack([rng.uniform(0, W, nb), rng.uniform(0, H, nb)], 1)
    corr = np.zeros(N, CORR_DTYPE)
    corr["xw"] = Xw; corr["uv"] = uv.astype(np.float32)
    corr["sigma2"] = SIGMA2[rng.integers(0, 8, N)] if octaves else 1.0
    corr["tag"] = np.sort(rng.permutation(max(2 * N, 1))[:N])
    prob = np.zeros(1, PROBLEM_DTYPE)
    prob["K"] = K; prob["seed"] = int(rng.integers(1, 2 ** 62)); prob["start_iteration"] = start; prob["n_iterations"] = n_iterations
    pr = dict(name=name or "seed%d_n%d" % (seed, N), corr=corr, prob=prob, R=R, t=t, bad=bad, **dict(DEFAULTS, **params))
    return pr


def reseed(pr, seed):
    q = dict(pr); q["prob"] = pr["prob"].copy(); q["prob"]["seed"] = seed
    return q


def resumed(pr, start, n_iterations=5):
    q = dict(pr); q["prob"] = pr["prob"].copy(); q["prob"]["start_iteration"] = start; q["prob"]["n_iterations"] = n_iterations
    q["name"] = pr["name"] + "_from%d" % start
    return q


def search_seed(pr, want, tries=400, first=1):
    """The first sampler seed (from `first`) for which want(result, inliers, info) holds under the oracle; the crafted branches that depend on
    which samples are drawn are reached this way, deterministically."""
    for s in range(first, first + tries):
        q = reseed(pr, s)
        r, inl, info = iterate(q)
        if want(r, inl, info):
            return q
    raise AssertionError("%s: no seed in [%d, %d) reaches the wanted branch" % (pr["name"], first, first + tries))


# ---- numpy / float64 restatement of EPnP (numpy.linalg.svd), independent of sd_pnp_math.h ----
def epnp_numpy(Xw, uv, K):
    Xw = np.asarray(Xw, np.float64); uv = np.asarray(uv, np.float64); fu, fv, uc, vc = (float(v) for v in K)
    n = len(Xw)
    c0 = Xw.mean(0)
    P0 = Xw - c0
    U, d, _ = np.linalg.svd(P0.T @ P0)
    cws = np.vstack([c0] + [c0 + np.sqrt(d[i] / n) * U[:, i] for i in range(3)])
    CC = (cws[1:] - cws[0]).T
    al = np.zeros((n, 4)); al[:, 1:] = (Xw - cws[0]) @ np.linalg.pinv(CC).T; al[:, 0] = 1 - al[:, 1:].sum(1)
    M = np.zeros((2 * n, 12))
    for i in range(4):
        M[0::2, 3 * i] = al[:, i] * fu; M[0::2, 3 * i + 2] = al[:, i] * (uc - uv[:, 0])
        M[1::2, 3 * i + 1] = al[:, i] * fv; M[1::2, 3 * i + 2] = al[:, i] * (vc - uv[:, 1])
    Um, _, _ = np.linalg.svd(M.T @ M)
    ut = Um.T
    v = [ut[11 - i].reshape(4, 3) for i in range(4)]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = [[vi[a] - vi[b] for a, b in pairs] for vi in v]
    L = np.zeros((6, 10))
    for i in range(6):
        d_ = [dv[k][i] for k in range(4)]
        L[i] = [d_[0] @ d_[0], 2 * d_[0] @ d_[1], d_[1] @ d_[1], 2 * d_[0] @ d_[2], 2 * d_[1] @ d_[2], d_[2] @ d_[2], 2 * d_[0] @ d_[3],
                2 * d_[1] @ d_[3], 2 * d_[2] @ d_[3], d_[3] @ d_[3]]
    rho = np.array([np.sum((cws[a] - cws[b]) ** 2) for a, b in pairs])

    def gauss_newton(b):
        b = np.array(b, np.float64)
        for _ in range(5):
            A = np.zeros((6, 4)); r = np.zeros(6)
            for i in range(6):
                l = L[i]
                A[i] = [2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3], l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3],
                        l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3], l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3]]
                r[i] = rho[i] - (l[0] * b[0] ** 2 + l[1] * b[0] * b[1] + l[2] * b[1] ** 2 + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] + l[5] * b[2] ** 2 +
                                 l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] ** 2)
            b = b + np.linalg.lstsq(A, r, rcond=None)[0]
        return b

    def r_and_t(b):
        ccs = sum(b[i] * v[i] for i in range(4))
        pcs = al @ ccs
        if pcs[0, 2] < 0:
            ccs, pcs = -ccs, -pcs
        pc0, pw0 = pcs.mean(0), Xw.mean(0)
        U_, _, Vt = np.linalg.svd((pcs - pc0).T @ (Xw - pw0))
        R = U_ @ Vt
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ pw0
        p, _ = project(R, t, Xw, (fu, fv, uc, vc))
        return R, t, np.mean(np.sqrt(((p - uv) ** 2).sum(1)))

    out = []
    b4 = np.linalg.lstsq(L[:, [0, 1, 3, 6]], rho, rcond=None)[0]
    s = np.sqrt(abs(b4[0])); sg = -1.0 if b4[0] < 0 else 1.0
    out.append(r_and_t(gauss_newton([s, sg * b4[1] / s, sg * b4[2] / s, sg * b4[3] / s])))
    b3 = np.linalg.lstsq(L[:, [0, 1, 2]], rho, rcond=None)[0]
    b0 = np.sqrt(abs(b3[0])); b1 = np.sqrt(-b3[2]) if (b3[0] < 0 and b3[2] < 0) else (np.sqrt(b3[2]) if (b3[0] >= 0 and b3[2] > 0) else 0.0)
    out.append(r_and_t(gauss_newton([-b0 if b3[1] < 0 else b0, b1, 0, 0])))
    b5 = np.linalg.lstsq(L[:, [0, 1, 2, 3, 4]], rho, rcond=None)[0]
    b0 = np.sqrt(abs(b5[0])); b1 = np.sqrt(-b5[2]) if (b5[0] < 0 and b5[2] < 0) else (np.sqrt(b5[2]) if (b5[0] >= 0 and b5[2] > 0) else 0.0)
    b0 = -b0 if b5[1] < 0 else b0
    out.append(r_and_t(gauss_newton([b0, b1, b5[3] / b0, 0])))
    N = 0
    if out[1][2] < out[0][2]:
        N = 1
    if out[2][2] < out[N][2]:
        N = 2
    return out[N][0], out[N][1], N + 1


def pack(problems):
    """(corr_offset (n + 1,), corr (E,), problems (n,)) of a list of problems sharing their SetRansacParameters arguments."""
    off = np.zeros(len(problems) + 1, np.int32)
    off[1:] = np.cumsum([len(p["corr"]) for p in problems])
    corr = np.concatenate([np.ascontiguousarray(p["corr"], CORR_DTYPE) for p in problems]) if problems else np.zeros(0, CORR_DTYPE)
    probs = np.concatenate([np.ascontiguousarray(p["prob"], PROBLEM_DTYPE).reshape(1) for p in problems]) if problems else np.zeros(0, PROBLEM_DTYPE)
    return off, corr, probs


def group_key(pr):
    return _args(pr)


# ---- the crafted problems ----
def _exact(seed, n_in, n_out, name, **kw):
    """n_in points exactly on the pose plus n_out uniform outliers, every octave 0 (sigma2 = 1): a sample of four inliers gives a count of
    exactly n_in and Refine gives n_in again."""
    pr = make_problem(seed, n_in + n_out, outliers=n_out / float(n_in + n_out), noise=0.0, octaves=False, name=name, **kw)
    return pr


def two_structures(seed, n_true, n_decoy, n_noise, name, **kw):
    """n_true points on one pose, n_decoy on another, n_noise uniform outliers (all sigma2 = 1), shuffled."""
    a = make_problem(seed, n_true, octaves=False)
    b = make_problem(seed + 1000, n_decoy, octaves=False)
    c = make_problem(seed + 2000, max(n_noise, 1), outliers=1.0, octaves=False)
    corr = np.concatenate([a["corr"], b["corr"], c["corr"][:n_noise]])
    rng = np.random.default_rng(seed + 3000)
    perm = rng.permutation(len(corr))
    corr = corr[perm]; corr["tag"] = np.arange(len(corr)) * 2
    pr = dict(a, name=name, corr=corr, structure=np.concatenate([np.zeros(n_true, int), np.ones(n_decoy, int), np.full(n_noise, 2)])[perm], **kw)
    pr["bad"] = pr["structure"] != 0
    return pr


def bound_scan_problem(count=512, seed=77):
    """`count` items whose error2 under the pose of ITERATION 1 lies one f32 step to either side of sigma2 * th2 (alternating, at every
    octave), placed by bisection of uv[0] under the oracle; plus one item with error2 == bound (inf == inf).  The items are not in
    iteration 1's sample, so moving them does not move its pose.  -> (problem, expected mask of iteration 1 over the scan items)."""
    pr = make_problem(seed, count + 40, octaves=True, name="bound_scan", min_inliers=10, epsilon=0.02, max_iterations=8)
    N = len(pr["corr"])
    smp = set(int(v) for v in sample_literal(int(pr["prob"]["seed"][0]), 1, N))
    _, poses, _ = hypotheses(pr, 1)
    K = pr["prob"]["K"][0]
    items = [i for i in range(N) if i not in smp][:count]
    want = np.zeros(N, np.uint8); scan = np.zeros(N, bool)
    rows = rows_of(pr)
    for k, i in enumerate(items):
        rows[i, 5] = np.float32(SIGMA2[k % 8]) * np.float32(pr["th2"]); pr["corr"]["sigma2"][i] = SIGMA2[k % 8]
        inside = lambda u: check(poses[0], np.concatenate([rows[i, :3], [u, rows[i, 4], rows[i, 5]]]).astype(np.float32)[None], K)[0] == 1
        lo = np.float32(rows[i, 3]); hi = np.float32(lo + 3.0 * np.sqrt(rows[i, 5]))
        assert inside(lo) and not inside(hi)
        while np.nextafter(lo, np.float32(np.inf)) < hi:
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if inside(mid):
                lo = mid
            else:
                hi = mid
        u = lo if k % 2 == 0 else hi
        pr["corr"]["uv"][i, 0] = u; want[i] = 1 if k % 2 == 0 else 0; scan[i] = True
    j = [i for i in range(N) if i not in smp and not scan[i]][0]
    pr["corr"]["uv"][j, 0] = np.inf; pr["corr"]["sigma2"][j] = np.inf; pr["equal_item"] = j
    pr["scan"] = scan; pr["scan_want"] = want
    return pr


_cases = None


def decision(pr, order=0, contract="off"):
    r, inl, _ = iterate(pr, order=order, contract=contract)
    return (int(r["kind"]), int(r["iteration"]), int(r["n_inliers"]), inl.tobytes())


def stable(pr):
    """True when kind, iteration, n_inliers and the mask are the same under both summation orders and both contraction settings."""
    d = decision(pr)
    return all(decision(pr, o, c) == d for o, c in ((1, "off"), (0, "fast"), (1, "fast")))


def pick(build, want=None, seeds=range(1, 200)):
    """The first seed whose problem is stable() and reaches the wanted branch under the oracle."""
    for s in seeds:
        pr = build(s)
        if pr is None:
            continue
        if want is not None and not want(*iterate(pr)):
            continue
        if stable(pr):
            return pr
    raise AssertionError("no seed gives a stable problem on the wanted branch")


def ransac_cases():
    """The crafted problems; `expect` names the branch each was made for (tests/test_pnp_oracle.py pins it under the oracle).  Every one is
    chosen (by a deterministic search over seeds) so that the oracle keeps its decision under both orders and both contraction settings."""
    global _cases
    if _cases is not None:
        return _cases
    cs = []

    def add(pr, expect):
        pr["expect"] = expect
        cs.append(pr)

    add(make_problem(11, 3, name="size_3"), dict(kind=0, iterations=0))                                # below the minimal set
    # (a seed whose three beta approximations do not tie in reprojection error: with a tie FMA picks another of the four-point solutions
    # and the oracle's own spread of the pose is 5e-2)
    add(pick(lambda s: (lambda q: q if spread(q) < 1e-5 else None)(make_problem(s, 4, name="size_4_min4", octaves=False, min_inliers=4)),
             lambda r, i, f: f["ties"] > 0),
        dict(kind=2, iterations=5, max_its=1, ties=True))                                              # N == min_inliers: nIterations = 1, five run
    add(pick(lambda s: make_problem(s, 5, name="size_5_min4", octaves=False, min_inliers=4)), dict(kind=1))
    for n in (63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, MAX_N):
        add(pick(lambda s: make_problem(20 + s, n, outliers=0.3, noise=0.0 if n != 65 else 0.2, name="size_%d" % n)), dict(kind=1))
    add(make_problem(14, 8, name="n_below_min_inliers"), dict(kind=0, iterations=0))
    add(pick(lambda s: make_problem(s, 100, outliers=0.0, noise=0.2, name="outliers_0"), lambda r, i, f: r["iteration"] == 1), dict(kind=1, iteration=1))
    add(pick(lambda s: make_problem(s, 100, outliers=0.3, noise=0.2, name="outliers_30")), dict(kind=1))
    add(pick(lambda s: make_problem(s, 100, outliers=0.6, noise=0.0, name="outliers_60", epsilon=0.3)), dict(kind=1))
    add(pick(lambda s: make_problem(s, 100, outliers=1.0, name="outliers_100")), dict(kind=0, at_end=True))
    # success in the middle / at `end`
    add(pick(lambda s: reseed(make_problem(34, 60, outliers=0.45, name="found_middle", epsilon=0.4), s),
             lambda r, i, f: r["kind"] == 1 and 3 <= r["iteration"] < r["max_its"] - 8), dict(kind=1))
    add(pick(lambda s: reseed(make_problem(35, 60, outliers=0.45, name="found_at_end", epsilon=0.4, max_iterations=6), s),
             lambda r, i, f: r["kind"] == 1 and r["iteration"] == 6 == r["max_its"]), dict(kind=1, at_end=True))
    # counts exactly min_inliers - 1 / min_inliers / min_inliers + 1 (min_inliers = 10 of N = 20)
    add(pick(lambda s: _exact(s, 9, 11, "count_min_minus_1"), lambda r, i, f: f["below_min"] > 0), dict(kind=0, at_end=True, below_min=True))
    add(pick(lambda s: _exact(s, 10, 10, "count_equals_min"), lambda r, i, f: f["ties"] > 0 and r["kind"] == 2),
        dict(kind=2, at_end=True, ties=True, refined=10))                                              # Refine gives exactly min_inliers: strict > fails
    add(pick(lambda s: _exact(s, 11, 9, "count_min_plus_1"), lambda r, i, f: r["kind"] == 1), dict(kind=1, refined=11))
    # a best whose Refine fails while a later, larger best succeeds
    add(pick(lambda s: reseed(two_structures(50, 20, 12, 8, "decoy_then_true", epsilon=0.3, min_inliers=12), s),
             lambda r, i, f: r["kind"] == 1 and f["refine_fails"] >= 1 and f["distinct_refines"] >= 2 and r["n_inliers"] == 20, range(1, 600)),
        dict(kind=1, refine_fails=True))

    # a later hypothesis below the best whose own mask would refine: Refine must still take the best mask
    def cur(s):
        q = make_problem(s, 30, outliers=0.4, noise=1.6, octaves=False, name="refine_takes_best_mask", epsilon=0.3, min_inliers=9)
        return q if not same_result(iterate(q)[0], iterate(q, twin="refine_current")[0]) else None
    add(pick(cur, None, range(60, 400)), dict(refine_fails=True))

    # resumed calls: one that returns at once from the same best, one that first meets a new best
    def again(new_best):
        def build(s):
            q = reseed(make_problem(36, 80, outliers=0.5, noise=0.0 if not new_best else 1.2, name="resume", epsilon=0.3, octaves=False), s)
            r = iterate(q)[0]
            if r["kind"] != 1 or r["iteration"] + 5 > r["max_its"]:
                return None
            q2 = resumed(q, int(r["iteration"]))
            r2 = iterate(q2)[0]
            ok = r2["kind"] == 1 and ((r2["best_iteration"] > r["iteration"]) if new_best else (r2["best_iteration"] == r["best_iteration"]))
            q2["first_call"] = q
            return q2 if ok and stable(q) else None
        return build
    q = pick(again(False)); q["name"] = "resume_same_best"
    add(q, dict(kind=1, same_best=True))
    q = pick(again(True), None, range(1, 600)); q["name"] = "resume_new_best"
    add(q, dict(kind=1, new_best=True))
    add(bound_scan_problem(), dict(scan=True))
    # degenerate geometry
    add(pick(lambda s: make_problem(s, 40, planar=1e-12, noise=0.0, name="planar")), dict())
    col = make_problem(71, 20, name="collinear", octaves=False)
    col["corr"]["xw"] = (col["corr"]["xw"][0][None] + np.linspace(0, 1, 20, dtype=np.float32)[:, None] * (col["corr"]["xw"][1] - col["corr"]["xw"][0])[None])
    add(col, dict())
    co = make_problem(72, 4, name="coincident", octaves=False, min_inliers=4)
    co["corr"]["xw"][:] = co["corr"]["xw"][0]; co["corr"]["uv"][:] = co["corr"]["uv"][0]
    add(co, dict(kind=0, flag=F_B4_ZERO))

    def z0(s):
        q = make_problem(s, 40, name="z_zero")
        q["corr"]["xw"][5] = (-(q["R"].T @ q["t"])).astype(np.float32)                 # the camera centre: Xc = Yc = Zc ~ 0
        return q
    add(pick(z0), dict(kind=1, outside=5))

    def nan(s):
        q = make_problem(s, 40, name="nan_coordinate")
        q["corr"]["xw"][7, 0] = np.nan
        return q
    add(pick(nan), dict(kind=1, outside=7))
    _cases = cs
    return cs


def field_bytes(v):
    return np.ascontiguousarray(v).tobytes()


def same_result(a, b):
    return a.tobytes() == b.tobytes()


def spread(pr):
    """The oracle's own spread of a case's pose: the largest |difference| of a finite Tcw entry between the sequential / contraction-off
    result and the three other (order, contraction) settings."""
    ref = iterate(pr)[0]["Tcw"].astype(np.float64)
    s = 0.0
    for o, c in ((1, "off"), (0, "fast"), (1, "fast")):
        T = iterate(pr, order=o, contract=c)[0]["Tcw"].astype(np.float64)
        fin = np.isfinite(ref) & np.isfinite(T)
        if fin.any():
            s = max(s, float(np.abs(T[fin] - ref[fin]).max()))
    return s


def random_problem(rng):
    """A random draw of the fuzz sweep: size, outlier rate, noise, depth range, near-planar scenes."""
    N = int(rng.choice([rng.integers(4, 40), rng.integers(40, 300), rng.integers(300, 1500)], p=[0.3, 0.55, 0.15]))
    near, far = float(rng.uniform(1.0, 8.0)), float(rng.uniform(10.0, 60.0))
    return make_problem(int(rng.integers(1 << 30)), N, outliers=float(rng.choice([0.0, 0.2, 0.4, 0.6, 0.9])), noise=float(rng.choice([0.0, 0.05, 0.1, 0.2])),
                        K=K_KITTI if rng.integers(2) else K_TUM, depth=(near, far), planar=float(rng.choice([0.0, 0.0, 0.0, 1e-3, 1e-9])),
                        n_iterations=int(rng.choice([1, 5, 40])), min_inliers=int(rng.choice([4, 10])), epsilon=float(rng.choice([0.3, 0.5])),
                        max_iterations=int(rng.choice([30, 300])))
