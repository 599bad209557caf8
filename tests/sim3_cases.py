"""Shared by test_sim3_oracle.py, test_gpu_sim3.py, tools/fuzz_sim3.py and tools/bench_sim3.py: the Sim3Solver CPU oracle
(tests/cpp/sim3_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory) and seeded crafted RANSAC problems in
plain numpy.

A problem is dict(corr (CORR_DTYPE), prob (PROBLEM_DTYPE scalar), min_inliers, max_iterations, probability, expect) where expect names
the branch the case was made for: "none" (N < min_inliers: no hypothesis), "found", "found_first" (at iteration 1), "found_last" (only
at the last allowed iteration), "exhausted", and optionally truth = (s, R, t) of the generating similarity.
Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR_DTYPE = np.dtype([("xw1", "<f4", (3,)), ("xw2", "<f4", (3,)), ("sigma2_1", "<f4"), ("sigma2_2", "<f4"), ("tag", "<i4")])      # sd_sim3_corr
PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("fix_scale", "<i4"),
                          ("reserved", "<i4"), ("seed", "<u8")])                                                                   # sd_sim3_problem
RESULT_DTYPE = np.dtype([("found", "<i4"), ("no_more", "<i4"), ("iteration", "<i4"), ("n_inliers", "<i4"), ("max_its", "<i4"),
                         ("reserved", "<i4"), ("T12", "<f4", (16,)), ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4")])   # sd_sim3_result
assert CORR_DTYPE.itemsize == 36 and PROBLEM_DTYPE.itemsize == 176 and RESULT_DTYPE.itemsize == 140

K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)        # fx fy cx cy
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2              # mvLevelSigma2 of the default pyramid
LDS_CHUNK, MAX_N, MAX_ITS = 512, 4096, 4096                                    # the header's staging chunk and caps
BRANCH = {0: "none", 1: "found", 2: "exhausted"}

_oracles = {}


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast and FMA (to count the decisions it changes)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="sim3_oracle_")
        so = os.path.join(d, "libsim3_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []              # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "sim3_oracle.cpp")])
        L = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        L.sd_sim3_oracle_find.argtypes = [vp, vp, i, C.c_double, i, i, vp, vp, vp]
        L.sd_sim3_oracle_find_range.argtypes = [i, i, vp, vp, vp, C.c_double, i, i, vp, vp, vp]
        L.sd_sim3_oracle_sample.argtypes = [C.c_uint64, i, i, vp]
        L.sd_sim3_oracle_remove.argtypes = [vp, i, vp]
        L.sd_sim3_oracle_horn.argtypes = [vp, vp, i, vp]
        L.sd_sim3_oracle_check.argtypes = [vp, vp, i, vp, vp, vp, vp]
        L.sd_sim3_oracle_max_its.argtypes = [C.c_double, i, i, i]
        _oracles[contract] = L
    return _oracles[contract]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def find(pr, contract="off"):
    """Sim3Solver::find of one problem on the CPU: (result (RESULT_DTYPE scalar), inliers (N,) u8, info (4,) int64)."""
    c = np.ascontiguousarray(pr["corr"], CORR_DTYPE)
    p = np.ascontiguousarray(pr["prob"], PROBLEM_DTYPE).reshape(1)
    res = np.zeros(1, RESULT_DTYPE); inl = np.zeros(max(len(c), 1), np.uint8); info = np.zeros(4, np.int64)
    oracle(contract).sd_sim3_oracle_find(_p(p), _p(c), len(c), float(pr["probability"]), int(pr["min_inliers"]), int(pr["max_iterations"]),
                                         _p(res), _p(inl), _p(info))
    return res[0], inl[:len(c)], info


def find_packed(off, corr, probs, probability, min_inliers, max_iterations, threads=1):
    """find() of every problem of packed tables (pack()): -> (results (n,), inliers (E,), info (n, 4)).  The tables are marshalled once;
    each of `threads` host threads then makes ONE call that loops over a contiguous chunk of problems in C (ctypes drops the GIL for
    its duration), so the threads run side by side."""
    from concurrent.futures import ThreadPoolExecutor
    n = len(probs)
    res = np.zeros(max(n, 1), RESULT_DTYPE); inl = np.zeros(max(len(corr), 1), np.uint8); info = np.zeros((max(n, 1), 4), np.int64)
    L = oracle()
    args = (_p(off), _p(corr), _p(probs), float(probability), int(min_inliers), int(max_iterations), _p(res), _p(inl), _p(info))
    cuts = [n * k // threads for k in range(threads + 1)]
    run = lambda k: L.sd_sim3_oracle_find_range(cuts[k], cuts[k + 1], *args)
    if threads == 1:
        run(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(run, range(threads)))
    return res[:n], inl[:len(corr)], info[:n]


def horn(x1, x2, fix_scale, contract="off"):
    """ComputeSim3 of three camera-frame pairs: dict(T12 (4,4), T21 (4,4), R (3,3), t (3,), s)."""
    a = np.ascontiguousarray(x1, np.float32).reshape(9); b = np.ascontiguousarray(x2, np.float32).reshape(9)
    out = np.zeros(45, np.float32)
    oracle(contract).sd_sim3_oracle_horn(_p(a), _p(b), int(fix_scale), _p(out))
    return dict(T12=out[:16].reshape(4, 4), T21=out[16:32].reshape(4, 4), R=out[32:41].reshape(3, 3), t=out[41:44], s=out[44])


def check(pr, T12, T21, contract="off"):
    """CheckInliers of a given transform: (count, err (N, 2) f32, inlier (N,) u8)."""
    c = np.ascontiguousarray(pr["corr"], CORR_DTYPE)
    p = np.ascontiguousarray(pr["prob"], PROBLEM_DTYPE).reshape(1)
    a = np.ascontiguousarray(T12, np.float32).reshape(16); b = np.ascontiguousarray(T21, np.float32).reshape(16)
    err = np.zeros((max(len(c), 1), 2), np.float32); inl = np.zeros(max(len(c), 1), np.uint8)
    k = oracle(contract).sd_sim3_oracle_check(_p(p), _p(c), len(c), _p(a), _p(b), _p(err), _p(inl))
    return k, err[:len(c)], inl[:len(c)]


# ---------------------------------------------------------------- the sampler's closed form (what the kernel uses)
_M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def draws(seed, iteration, N):
    base = (splitmix64(seed) + (iteration << 2)) & _M64
    return [splitmix64((base + d) & _M64) % (N - d) for d in range(3)]


def removal_closed_form(r, N):
    """The three indices the swap-with-back removal (Sim3Solver.cc:163-177) yields for draws r[k] < N - k, without a vector."""
    first = lambda j: N - 1 if j == r[0] else j          # the vector after the first removal
    return [r[0], first(r[1]), first(N - 2) if r[2] == r[1] else first(r[2])]


def removal_literal(r, N):
    rr = np.array(r, np.int32); out = np.zeros(3, np.int32)
    oracle().sd_sim3_oracle_remove(_p(rr), N, _p(out))
    return [int(v) for v in out]


def sample_literal(seed, iteration, N):
    out = np.zeros(3, np.int32)
    oracle().sd_sim3_oracle_sample(C.c_uint64(seed), iteration, N, _p(out))
    return [int(v) for v in out]


# ---------------------------------------------------------------- geometry
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R; T[:3, 3] = t
    return T


def horn_f64(x1, x2, fix_scale):
    """Horn 1987 in float64 numpy (numpy's symmetric eigensolver): x1 ~ s R x2 + t for (n, 3) arrays -> (s, R, t)."""
    x1 = np.asarray(x1, np.float64); x2 = np.asarray(x2, np.float64)
    o1, o2 = x1.mean(0), x2.mean(0)
    a, b = (x1 - o1).T, (x2 - o2).T
    M = b @ a.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    q = V[:, 3]
    ang = 2 * np.arctan2(np.linalg.norm(q[1:]), q[0])
    R = rodrigues(ang * q[1:] / np.linalg.norm(q[1:])) if np.linalg.norm(q[1:]) > 0 else np.eye(3)
    P3 = R @ b
    s = 1.0 if fix_scale else float((a * P3).sum() / (P3 * P3).sum())
    return s, R, o1 - s * R @ o2


def make_problem(seed, N, s=1.0, fix_scale=False, outliers=0.0, noise=0.0, min_inliers=20, max_iterations=300, probability=0.99,
                 K1=K_KITTI, K2=K_KITTI, identity=False, ransac_seed=None):
    """N correspondences of one physical scene seen from two keyframes whose maps differ by the similarity x1c = s R x2c + t.
    outliers: share of correspondences whose first point is replaced by an unrelated one; noise: Gaussian noise on the camera-frame
    points (metres).  identity: both poses and the similarity are the identity (every entry exact in f32)."""
    rng = np.random.default_rng([seed, N, int(round(s * 1000)), int(fix_scale), int(round(outliers * 100)), int(identity)])
    x2c = np.stack([rng.uniform(-6, 6, N), rng.uniform(-2, 2, N), rng.uniform(5, 25, N)], 1)
    if identity:
        R12, t12, s = np.eye(3), np.zeros(3), 1.0
        T1 = T2 = np.eye(4)
    else:
        R12 = rodrigues(rng.normal(0, 0.03, 3)); t12 = rng.normal(0, 0.3, 3)
        T1 = pose(rodrigues(rng.normal(0, 0.4, 3)), rng.normal(0, 3, 3)); T2 = pose(rodrigues(rng.normal(0, 0.4, 3)), rng.normal(0, 3, 3))
    x1c = s * x2c @ R12.T + t12
    if noise:
        x1c = x1c + rng.normal(0, noise, x1c.shape)
    bad = np.zeros(N, bool)
    nb = int(round(outliers * N))
    if nb:
        bad[rng.choice(N, nb, replace=False)] = True
        x1c[bad] = np.stack([rng.uniform(-6, 6, nb), rng.uniform(-2, 2, nb), rng.uniform(5, 25, nb)], 1) * s
    T1 = T1.astype(np.float32).astype(np.float64); T2 = T2.astype(np.float32).astype(np.float64)
    w1 = (x1c - T1[:3, 3]) @ T1[:3, :3]; w2 = (x2c - T2[:3, 3]) @ T2[:3, :3]            # R^T (x - t)
    c = np.zeros(N, CORR_DTYPE)
    c["xw1"] = w1; c["xw2"] = w2
    c["sigma2_1"] = SIGMA2[rng.integers(0, 8, N)]; c["sigma2_2"] = SIGMA2[rng.integers(0, 8, N)]
    c["tag"] = np.sort(rng.choice(max(2 * N, 1), N, replace=False)) if N else 0
    p = np.zeros((), PROBLEM_DTYPE)
    p["Tcw1"] = T1.reshape(16); p["Tcw2"] = T2.reshape(16); p["K1"] = K1; p["K2"] = K2; p["fix_scale"] = int(fix_scale)
    p["seed"] = np.uint64(splitmix64(seed * 1000003 + N) if ransac_seed is None else ransac_seed)
    return dict(corr=c, prob=p, min_inliers=min_inliers, max_iterations=max_iterations, probability=probability, truth=(s, R12, t12), bad=bad)


def _expect(pr, what, name):
    pr["expect"] = what; pr["name"] = name
    return pr


def _search_seed(pr, want, tries=4000):
    """The first RANSAC seed (from a fixed sequence) for which the oracle's result satisfies `want`."""
    for k in range(tries):
        pr["prob"]["seed"] = np.uint64(splitmix64(0xC0FFEE + k))
        r, _, _ = find(pr)
        if want(r):
            return pr
    raise AssertionError("no seed found for %s" % pr.get("name"))


def error_bound_problem():
    """Identity poses and similarity with fix_scale: every hypothesis is exactly the identity (M is symmetric, so N's first row is
    (trace, 0, 0, 0) and no rotation touches it), hence err1 of a correspondence is just the squared pixel distance of its two points.
    25 exact pairs (more than min_inliers = 20, so iteration 1 succeeds) and four probes on level 0 whose second point is displaced
    along u so that err1 is about 8.9, 9.0, 9.1 and 9.2 px^2: the bound is (size_t)(9.210 * 1) = 9, not 9.21."""
    pr = make_problem(901, 29, identity=True, fix_scale=True)
    c = pr["corr"]
    c["xw2"] = c["xw1"]
    c["sigma2_1"][25:] = SIGMA2[0]; c["sigma2_2"][25:] = SIGMA2[7]
    fx = np.float64(K_KITTI[0])
    for k, e in enumerate((8.9, 9.0, 9.1, 9.2)):
        z = np.float64(c["xw1"][25 + k][2])
        c["xw2"][25 + k][0] = np.float32(np.float64(c["xw1"][25 + k][0]) + np.sqrt(e) * z / fx)
    pr["probes"] = {8.9: 25, 9.0: 26, 9.1: 27, 9.2: 28}
    return _expect(pr, "found_first", "error_bound")


def bound_scan(geom, count=32):
    """`count` consecutive f32 values of a probe's displaced coordinate around the point where its err1 crosses the level-0 bound,
    placed by bisection with the oracle: returns (problem, probe row, [f32 values])."""
    pr = error_bound_problem()
    c = pr["corr"]
    row = 25
    rng = np.random.default_rng([77, geom])
    c["xw1"][row] = (rng.uniform(-5, 5), rng.uniform(-2, 2), rng.uniform(5, 25))
    c["xw2"][row] = c["xw1"][row]
    I = np.eye(4, dtype=np.float32)

    def inl(x):
        c["xw2"][row][0] = x
        return bool(check(pr, I, I)[2][row])
    lo = np.float32(c["xw1"][row][0]); hi = np.float32(lo + np.float32(4.0 * c["xw1"][row][2] / K_KITTI[0]))      # 0 px (in) and 4 px (out)
    assert inl(lo) and not inl(hi)
    while True:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if inl(mid):
            lo = mid
        else:
            hi = mid
    vals = [lo]
    for _ in range(count // 2 - 1):
        vals.insert(0, np.nextafter(vals[0], np.float32(-np.inf), dtype=np.float32))
    v = hi
    for _ in range(count // 2):
        vals.append(v); v = np.nextafter(v, np.float32(np.inf), dtype=np.float32)
    return pr, row, vals


_cases = None


def ransac_cases():
    """Every crafted RANSAC problem, in a fixed order (built once: two of them search seeds with the oracle)."""
    global _cases
    if _cases is not None:
        return _cases
    cs = []
    for N in (0, 2, 3, 4, 19, 20, 21, 63, 64, 65, 257, LDS_CHUNK + 1, MAX_N):
        what = "none" if N < 20 else ("exhausted" if N == 20 else "found_first")          # N == 20 == min_inliers: one iteration, 20 > 20 never holds
        cs.append(_expect(make_problem(1, N), what, "size_%d" % N))
    cs.append(_expect(make_problem(2, 3, min_inliers=2), "found_first", "three_points_min2"))
    cs.append(_expect(make_problem(2, 4, min_inliers=4), "exhausted", "min_inliers_equals_n"))
    for s in (0.5, 1.0, 2.0):
        for fix in (False, True):
            ok = (not fix) or s == 1.0
            cs.append(_expect(make_problem(3, 150, s=s, fix_scale=fix), "found_first" if ok else "exhausted", "clean_s%g_fix%d" % (s, fix)))
    cs.append(_expect(make_problem(4, 150, s=1.3, outliers=0.3, noise=0.002), "found", "outliers_30"))
    cs.append(_expect(make_problem(4, 150, s=0.8, outliers=0.6, noise=0.002), "found", "outliers_60"))
    last = make_problem(5, 40, outliers=0.4, max_iterations=8)
    last["name"] = "found_last"
    cs.append(_expect(_search_seed(last, lambda r: r["found"] and r["iteration"] == r["max_its"] == 8), "found_last", "found_last"))
    cs.append(_expect(make_problem(6, 60, outliers=1.0), "exhausted", "all_outliers"))          # ties on small counts: the latest wins
    co = make_problem(7, 30, identity=True)                 # (a + a + a) / 3 == a exactly for these values: Pr == 0, den == 0, s12 = 0 / 0
    co["corr"]["xw1"] = (1.0, -2.0, 8.0); co["corr"]["xw2"] = (1.0, -2.0, 8.0)
    cs.append(_expect(co, "exhausted", "coincident"))
    li = make_problem(8, 30, identity=True)
    tt = np.linspace(0, 1, 30)[:, None]
    li["corr"]["xw1"] = np.array([-3, -1, 6]) + tt * np.array([6.0, 2.0, 10.0]); li["corr"]["xw2"] = li["corr"]["xw1"]
    cs.append(_expect(li, None, "collinear"))                # the rotation about the line is free: whatever the restatement gives
    z0 = make_problem(9, 40, identity=True)
    z0["corr"]["xw2"] = z0["corr"]["xw1"]
    z0["corr"]["xw1"][5][2] = 0.0; z0["corr"]["xw2"][5][2] = 0.0                                # z = 0 in both cameras: 1 / 0
    z0["corr"]["xw1"][6][2] = 0.0                                                               # z = 0 in camera 1 only
    cs.append(_expect(z0, "found", "z_zero"))
    cs.append(error_bound_problem())
    cs.append(_expect(make_problem(10, 90, s=1.1, K1=K_KITTI, K2=K_TUM, noise=0.002), "found_first", "two_cameras"))
    _cases = cs
    return cs


def pack(problems):
    """(corr_offset (n + 1,) i32, corr, problems (n,) PROBLEM_DTYPE) of a list of problems."""
    off = np.zeros(len(problems) + 1, np.int32)
    off[1:] = np.cumsum([len(p["corr"]) for p in problems])
    corr = np.concatenate([p["corr"] for p in problems]) if len(problems) else np.zeros(0, CORR_DTYPE)
    probs = np.array([p["prob"] for p in problems], PROBLEM_DTYPE) if len(problems) else np.zeros(0, PROBLEM_DTYPE)
    return off, np.ascontiguousarray(corr), np.ascontiguousarray(probs)


def field_bytes(v):
    """The bytes of one result field, every NaN written as the one canonical quiet NaN: IEEE 754 leaves the sign and payload of the
    NaN an invalid operation (0 / 0) produces to the implementation, and x86 and gfx950 differ in the sign."""
    v = np.asarray(v)
    if v.dtype.kind == "f":
        v = np.where(np.isnan(v), np.array(np.nan, v.dtype), v)
    return v.tobytes()


def same_result(a, b):
    """Byte equality of two RESULT_DTYPE scalars (NaNs as field_bytes writes them)."""
    return all(field_bytes(a[f]) == field_bytes(b[f]) for f in RESULT_DTYPE.names)


def random_problem(rng):
    """A random problem for tools/fuzz_sim3.py."""
    N = int(rng.choice([int(rng.integers(0, 40)), int(rng.integers(40, 400)), int(rng.integers(400, 1500))]))
    return make_problem(int(rng.integers(1 << 30)), N, s=float(rng.uniform(0.5, 2.0)), fix_scale=bool(rng.integers(2)),
                        outliers=float(rng.choice([0.0, 0.3, 0.6, 0.9])), noise=float(rng.choice([0.0, 0.002, 0.02])),
                        min_inliers=int(rng.choice([20, 20, 5, 50])), max_iterations=int(rng.choice([300, 300, 17, 64])),
                        K2=K_TUM if rng.integers(2) else K_KITTI)


# ================================================================ ORBmatcher::SearchBySim3
# A scene is dict(name, kfs [two or more keyframe dicts of KeyFrameBuilder.build()], points (MP_DTYPE), pdesc (n, 32) u8, pairs [dict(k1,
# k2, s12, R12, t12, p1 (N1,) i32, p2 (N2,) i32, matched12 (N1,) i32)], th, expect {name: (pair, direction, source feature, branch,
# matched feature or -1)}).  The device tests write the keyframes over workspace slots (fuse_cases.Workspace), run sd_batch_assign_grid
# and ONE sd_batch_search_by_sim3 for all pairs; the CPU side runs the sequential oracle per pair.
import fuse_cases as fc                                                     # noqa: E402
import triangulate_cases as tc                                              # noqa: E402
from fuse_cases import MP_DTYPE                                             # noqa: E402
from triangulate_cases import CAM, F32, KP_DTYPE, KeyFrameBuilder, Levels   # noqa: E402

S3_BRANCHES = ["null_or_bad", "already", "z_neg", "u_below_min", "u_at_max", "v_below_min", "v_at_max", "not_finite", "dist_below", "dist_above",
               "empty", "no_octave", "too_far", "match"]
S3_COUNTERS = ["octave_below", "octave_above", "octave_lm1", "octave_l", "tie", "window_max", "agree_fail", "agree_ok", "cols_max"]
TH_SIM3 = 7.5
COL_W = 1241.0 / 64.0


def _search_binding(L):
    if not hasattr(L, "_s3"):
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.sd_sim3_oracle_search.argtypes = [i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, i, vp, i, vp, f, vp, vp, f, vp, vp, vp, vp, vp, vp]
        assert L.sd_sim3_oracle_counter_count() == len(S3_COUNTERS)
        L._s3 = True
    return L


def cpu_search(scene, contract="off", lv=None, cam=CAM):
    """Every pair of a scene through the sequential oracle -> ([(match12, vnMatch1, vnMatch2, nFound, branch1, branch2)], counters)."""
    L = _search_binding(oracle(contract))
    lv = lv or Levels()
    c = fc.cam_array(cam)
    pts = np.ascontiguousarray(scene["points"], MP_DTYPE); pd = np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1)
    cnt = np.zeros(len(S3_COUNTERS), np.int64)
    out = []
    for pr in scene["pairs"]:
        a, b = scene["kfs"][pr["k1"]], scene["kfs"][pr["k2"]]
        N1, N2 = len(a["kp"]), len(b["kp"])
        kp1 = np.ascontiguousarray(a["kp"], KP_DTYPE); kp2 = np.ascontiguousarray(b["kp"], KP_DTYPE)
        d1 = np.ascontiguousarray(a["desc"], np.uint8).reshape(-1); d2 = np.ascontiguousarray(b["desc"], np.uint8).reshape(-1)
        T1 = np.ascontiguousarray(a["Tcw"], F32).reshape(16); T2 = np.ascontiguousarray(b["Tcw"], F32).reshape(16)
        p1 = np.ascontiguousarray(pr["p1"], np.int32); p2 = np.ascontiguousarray(pr["p2"], np.int32); m = np.ascontiguousarray(pr["matched12"], np.int32)
        assert len(p1) == len(m) == N1 and len(p2) == N2
        R = np.ascontiguousarray(pr["R12"], F32).reshape(9); t = np.ascontiguousarray(pr["t12"], F32).reshape(3)
        v1 = np.zeros(max(N1, 1), np.int32); v2 = np.zeros(max(N2, 1), np.int32); m12 = np.zeros(max(N1, 1), np.int32)
        b1 = np.zeros(max(N1, 1), np.int32); b2 = np.zeros(max(N2, 1), np.int32)
        nf = L.sd_sim3_oracle_search(N1, _p(kp1), _p(d1), _p(T1), _p(p1), N2, _p(kp2), _p(d2), _p(T2), _p(p2), _p(m), _p(pts), _p(pd), len(pts),
                                     _p(c), lv.nlevels, _p(lv.scale), float(F32(pr["s12"])), _p(R), _p(t), scene.get("th", TH_SIM3), _p(v1), _p(v2),
                                     _p(m12), _p(b1), _p(b2), _p(cnt))
        out.append((m12[:N1].copy(), v1[:N1].copy(), v2[:N2].copy(), nf, b1[:N1].copy(), b2[:N2].copy()))
    return out, {k: int(v) for k, v in zip(S3_COUNTERS, cnt)}


def device_search(ws, scene, cam=CAM, upload=True):
    """One sd_batch_search_by_sim3 for all pairs of the scene -> [(match12 [:N1], vnMatch1 [:N1], vnMatch2 [:N2], nFound)]."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    prs = scene["pairs"]
    n = len(prs)
    t1 = np.full((max(n, 1), ws.cap), -1, np.int32); t2 = np.full((max(n, 1), ws.cap), -1, np.int32); tm = np.full((max(n, 1), ws.cap), -1, np.int32)
    for q, pr in enumerate(prs):
        t1[q, :len(pr["p1"])] = pr["p1"]; t2[q, :len(pr["p2"])] = pr["p2"]; tm[q, :len(pr["matched12"])] = pr["matched12"]
    d1, d2, dm = torch.from_numpy(t1).cuda(), torch.from_numpy(t2).cuda(), torch.from_numpy(tm).cuda()
    pts = np.ascontiguousarray(scene["points"], MP_DTYPE)
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda() if len(pts) else None
    d_desc = torch.from_numpy(np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1).copy()).cuda() if len(pts) else None
    kf = scene["kfs"]
    ws.b.search_by_sim3([pr["k1"] for pr in prs], [pr["k2"] for pr in prs], np.array([kf[pr["k1"]]["Tcw"] for pr in prs], F32).reshape(n, 16),
                        np.array([kf[pr["k2"]]["Tcw"] for pr in prs], F32).reshape(n, 16), [pr["s12"] for pr in prs],
                        np.array([pr["R12"] for pr in prs], F32).reshape(n, 9), np.array([pr["t12"] for pr in prs], F32).reshape(n, 3), cam,
                        d_pts.data_ptr() if d_pts is not None else None, d_desc.data_ptr() if d_desc is not None else None, d1.data_ptr(),
                        d2.data_ptr(), dm.data_ptr(), th=scene.get("th", TH_SIM3), n_points=len(pts))
    out = []
    for q, pr in enumerate(prs):
        m12, v1, v2, nf = ws.b.download_sim3_matches(q)
        N1, N2 = len(pr["p1"]), len(pr["p2"])
        assert (m12[N1:] == -1).all() and (v1[N1:] == -1).all() and (v2[N2:] == -1).all(), "rows beyond N must stay -1"
        out.append((m12[:N1].copy(), v1[:N1].copy(), v2[:N2].copy(), nf))
    del d1, d2, dm, d_pts, d_desc
    return out


def assert_same_search(scene, got, want):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        for k, what in enumerate(("match12", "vnMatch1", "vnMatch2")):
            assert g[k].tobytes() == w[k].tobytes(), "%s pair %d: %s differs at %r" % (scene["name"], q, what, np.nonzero(g[k] != w[k])[0][:8])
        assert g[3] == w[3], "%s pair %d: nFound %d vs %d" % (scene["name"], q, g[3], w[3])


def check_search_expectations(scene, results):
    for name, (pair, direction, i, branch, idx) in scene["expect"].items():
        r = results[pair]
        got = S3_BRANCHES[int(r[4 + direction][i])]
        assert got == branch, "%s: reached %s, made for %s" % (name, got, branch)
        assert int(r[1 + direction][i]) == idx, "%s: matched %d, meant %d" % (name, int(r[1 + direction][i]), idx)


class Sim3Scene:
    """Two keyframes and the similarity between their maps.  Direction 0 sends KF1's points into KF2, direction 1 the reverse."""

    def __init__(self, seed, s12=1.3, rot=(0.02, -0.01, 0.015), t12=(0.2, -0.1, 0.3), T1=None, T2=None, th=TH_SIM3, lv=None):
        self.rng = np.random.default_rng(7000 + seed)
        self.lv = lv or Levels()
        self.T = [np.asarray(tc.T1_DEFAULT if T1 is None else T1, np.float64), np.asarray(tc.neighbour_pose(tc.T1_DEFAULT, [0.4, 0.0, 0.1]) if T2 is None else T2, np.float64)]
        self.T = [t.astype(F32).astype(np.float64) for t in self.T]
        self.s12 = float(F32(s12)); self.R12 = rodrigues(rot).astype(F32); self.t12 = np.asarray(t12, F32)
        self.kf = [KeyFrameBuilder(self.T[0]), KeyFrameBuilder(self.T[1])]
        self.p = [[], []]
        self.points, self.pdesc, self.matched, self.expect, self.th = [], [], {}, {}, th
        self.strip = [0, 0]

    def world_of(self, direction, u, v, z):
        """The world point (in the SOURCE keyframe's map) that lands on pixel (u, v), depth z of the destination camera."""
        xd = np.array([(u - float(CAM["cx"])) / float(CAM["fx"]) * z, (v - float(CAM["cy"])) / float(CAM["fy"]) * z, z])
        R = self.R12.astype(np.float64); t = self.t12.astype(np.float64)
        xs = (R.T @ (xd - t)) / self.s12 if direction == 1 else self.s12 * R @ xd + t          # destination frame -> source frame
        return tc.to_world(self.T[direction], xs)[0], float(np.linalg.norm(xd))

    def point(self, direction, u, v, z=10.0, level=2, desc=None, min_distance=None, max_distance=None):
        X, dist = self.world_of(direction, u, v, z)
        r = np.zeros((), MP_DTYPE)
        r["xw"] = X; r["normal"] = (0, 0, 1); r["flags"] = 1
        mx = dist * float(self.lv.scale_factor) ** (level - 0.5) if max_distance is None else max_distance(dist)
        r["max_distance"] = mx
        r["min_distance"] = mx / float(self.lv.scale[-1]) if min_distance is None else min_distance(dist)
        self.points.append(r); self.pdesc.append(fc.rand_desc(self.rng) if desc is None else np.asarray(desc, np.uint8))
        return len(self.points) - 1

    def feature(self, k, u, v, desc, octave=2, point=-1):
        i = self.kf[k].add(u, v, desc, octave)
        self.p[k].append(point)
        return i

    def source(self, direction, point):
        """A source feature that only carries `point`: parked in a strip at the bottom of its image where no anchor looks, at octave 7."""
        n = self.strip[direction]; self.strip[direction] += 1
        return self.feature(direction, 15.0 + 9.0 * (n % 130), 352.0 + 6.0 * (n // 130), fc.rand_desc(self.rng), 7, point)

    def near(self, direction, p, du, dv, d, octave, u, v):
        """A destination feature at (u + du, v + dv) whose descriptor is d bits from point p's."""
        return self.feature(1 - direction, u + du, v + dv, fc.flipped(self.pdesc[p], d, self.rng), octave)

    def build(self, name):
        kfs = [k.build() for k in self.kf]
        N1 = len(kfs[0]["kp"])
        m = np.full(N1, -1, np.int32)
        for i1, v in self.matched.items():
            m[i1] = v
        pts = np.array(self.points, MP_DTYPE) if self.points else np.zeros(0, MP_DTYPE)
        pair = dict(k1=0, k2=1, s12=self.s12, R12=self.R12, t12=self.t12, p1=np.array(self.p[0], np.int32).reshape(-1),
                    p2=np.array(self.p[1], np.int32).reshape(-1), matched12=m)
        return dict(name=name, kfs=kfs, points=pts, pdesc=np.array(self.pdesc, np.uint8).reshape(len(pts), 32), pairs=[pair], th=self.th,
                    expect=self.expect)


def crafted_search_scene():
    """One anchor per `continue` and gate of SearchBySim3, in both directions, s12 = 1.3.  Anchors sit 75 px apart in the upper 300 rows;
    source features are parked below row 350."""
    S = Sim3Scene(1)
    ex = S.expect
    slot = [0]

    def anchor():
        i = slot[0]; slot[0] += 1
        return 60.0 + 75.0 * (i % 15), 30.0 + 50.0 * (i // 15)

    for d in (0, 1):
        tag = "d%d_" % d

        def single(name, branch, dist=10, octave=2, level=2, off=(0.0, 0.0), with_feature=True, uv=None, z=10.0, **kw):
            u, v = uv or anchor()
            p = S.point(d, u, v, z, level, **kw)
            f = S.near(d, p, off[0], off[1], dist, octave, u, v) if with_feature else -1
            i = S.source(d, p)
            ex[tag + name] = (0, d, i, branch, f if branch == "match" else -1)
            return i, f, p

        ex[tag + "null"] = (0, d, S.source(d, -1), "null_or_bad", -1)
        single("z_neg", "z_neg", z=-4.0)
        single("u_below_min", "u_below_min", uv=(-5.0, 100.0)); single("u_at_max", "u_at_max", uv=(1246.0, 100.0))
        single("v_below_min", "v_below_min", uv=(600.0, -5.0)); single("v_at_max", "v_at_max", uv=(600.0, 381.0))
        single("dist_below", "dist_below", min_distance=lambda dist: dist / 0.79)
        single("dist_above_min", "match", min_distance=lambda dist: dist / 0.81)
        single("dist_above", "dist_above", octave=0, max_distance=lambda dist: dist / 1.21, min_distance=lambda dist: dist / 8)
        single("dist_below_max", "match", octave=0, max_distance=lambda dist: dist / 1.19, min_distance=lambda dist: dist / 8)
        single("empty", "empty", with_feature=False)
        single("octave_lm2", "no_octave", octave=1, level=3); single("octave_lm1", "match", octave=2, level=3)
        single("octave_l", "match", octave=3, level=3); single("octave_lp1", "no_octave", octave=4, level=3)
        single("dist100", "match", dist=100); single("dist101", "too_far", dist=101)
        # a tie at distance 20: the feature added later (the higher index) lies one grid column to the left, is visited first and wins
        u, v = (10 + 8 * d + 0.5) * COL_W, 320.0
        p = S.point(d, u, v, 10.0, 2)
        f_lo = S.near(d, p, 3.0, 0.0, 20, 2, u, v); f_hi = S.near(d, p, -3.0, 0.0, 20, 2, u, v)
        assert fc.cell_of(u - 3.0, v)[0] < fc.cell_of(u + 3.0, v)[0] and f_hi > f_lo
        ex[tag + "tie"] = (0, d, S.source(d, p), "match", f_hi)
        # windows of 64 and 65 members; the nearest descriptor comes late in the walk
        for n in (64, 65):
            u, v = anchor(); p = S.point(d, u, v, 10.0, 2)
            for j in range(n):
                f = S.near(d, p, float(S.rng.uniform(-2, 2)), float(S.rng.uniform(-2, 2)), 11 if j == n - 4 else int(S.rng.integers(13, 60)), 2, u, v)
                if j == n - 4:
                    best = f
            ex[tag + "window_%d" % n] = (0, d, S.source(d, p), "match", best)
    # already matched through i1 (direction 0) and through idx2 (direction 1): both would match otherwise
    u, v = anchor(); p = S.point(0, u, v); f = S.near(0, p, 0, 0, 10, 2, u, v); i1 = S.source(0, p)
    u2, v2 = anchor(); q = S.point(1, u2, v2); S.near(1, q, 0, 0, 10, 2, u2, v2); i2 = S.source(1, q)
    S.matched[i1] = i2
    ex["already_i1"] = (0, 0, i1, "already", -1); ex["already_idx2"] = (0, 1, i2, "already", -1)
    # idx2 >= N2 and -2 mark vbAlreadyMatched1 only
    for name, val in (("idx2_beyond_n2", 100000), ("not_in_kf2", -2)):
        u, v = anchor(); p = S.point(0, u, v); S.near(0, p, 0, 0, 10, 2, u, v); i1 = S.source(0, p)
        S.matched[i1] = val
        ex[name] = (0, 0, i1, "already", -1)
    # agreement that holds: one physical point, seen at a1 in KF1 and a2 in KF2, a map point of each map on it
    a2 = anchor(); z2 = 9.0
    X1w, _ = S.world_of(0, a2[0], a2[1], z2)                          # in map 1
    x1c = X1w @ S.T[0][:3, :3].T + S.T[0][:3, 3]
    a1 = (float(CAM["fx"]) * x1c[0] / x1c[2] + float(CAM["cx"]), float(CAM["fy"]) * x1c[1] / x1c[2] + float(CAM["cy"]))
    assert 0 < a1[0] < 1241 and 0 < a1[1] < 300
    base = fc.rand_desc(S.rng)
    P1 = S.point(0, a2[0], a2[1], z2, 2, desc=fc.flipped(base, 5, S.rng))
    P2 = S.point(1, a1[0], a1[1], float(x1c[2]), 2, desc=fc.flipped(base, 5, S.rng))
    i1 = S.feature(0, a1[0], a1[1], fc.flipped(base, 8, S.rng), 2, P1); i2 = S.feature(1, a2[0], a2[1], fc.flipped(base, 8, S.rng), 2, P2)
    ex["agree_1"] = (0, 0, i1, "match", i2); ex["agree_2"] = (0, 1, i2, "match", i1)
    S.agree = (i1, i2)
    # agreement that fails: KF1's point finds i2b, but i2b's own point looks elsewhere in KF1 and finds another feature
    u, v = anchor(); p = S.point(0, u, v); u3, v3 = anchor(); q = S.point(1, u3, v3)
    i1b = S.source(0, p); other = S.near(1, q, 0, 0, 10, 2, u3, v3)
    i2b = S.feature(1, u, v, fc.flipped(S.pdesc[p], 10, S.rng), 2, q)
    ex["disagree_1"] = (0, 0, i1b, "match", i2b); ex["disagree_2"] = (0, 1, i2b, "match", other)
    S.disagree = i1b
    sc_ = S.build("crafted_search")
    sc_["agree"], sc_["disagree"] = S.agree, S.disagree
    return sc_


def window_columns(u, r):
    """Grid columns GetFeaturesInArea(u, ., r) spans, in f32 as the reference computes them."""
    wi = F32(64) / (CAM["mnMaxX"] - CAM["mnMinX"])
    lo = max(0, int(np.floor((F32(u) - CAM["mnMinX"] - F32(r)) * wi))); hi = min(63, int(np.ceil((F32(u) - CAM["mnMinX"] + F32(r)) * wi)))
    return hi - lo + 1


def wide_window_scene(cols):
    """A window of exactly `cols` (16 or 17) grid columns: th = 56 at level 5, the one matching feature in the window's last column."""
    S = Sim3Scene(2, th=56.0)
    r = float(F32(56.0) * S.lv.scale[5])
    for d in (0, 1):
        u = next(x for x in np.arange(500.0, 540.0, 0.25) if window_columns(x, r) == cols)
        v = 150.0
        p = S.point(d, u, v, 10.0, 5)
        f = S.near(d, p, r - 3.0, 0.0, 10, 5, u, v); S.near(d, p, -r + 3.0, 40.0, 30, 5, u, v)
        S.expect["d%d_cols_%d" % (d, cols)] = (0, d, S.source(d, p), "match", f)
    return S.build("wide_%d" % cols)


# ---------------------------------------------------------------- 1-ulp scans (the procedure of DESIGN Q31)
SEARCH_SCAN_KINDS = ("z_neg", "u_min", "u_max", "v_min", "v_max", "dist_min", "dist_max", "window_x", "window_y")
SEARCH_SCAN_GEOMETRIES, SEARCH_SCAN_POINTS = 4, 32
_I4 = np.eye(4)


def _scan_setup(kind, g):
    """(scene builder, point, field, index, start value (first outcome), end value (second outcome), branch of the second outcome)."""
    rng = np.random.default_rng([4242, SEARCH_SCAN_KINDS.index(kind), g])
    d = g & 1
    S = Sim3Scene(100 + g, s12=1.25, rot=(0, 0, 0), t12=(0.1, -0.05, 0.2), T1=_I4, T2=_I4)
    u, v, z = float(rng.uniform(300, 900)), float(rng.uniform(80, 280)), float(rng.uniform(6, 14))
    level = 0 if kind == "dist_max" else 2
    kw = {}
    if kind == "dist_max":
        kw = dict(max_distance=lambda dist: dist / 1.1, min_distance=lambda dist: dist / 8)
    p = S.point(d, u, v, z, level, **kw)
    S.near(d, p, 0.0, 0.0, 10, level, u, v)
    rec = S.points[p]
    r = float(F32(TH_SIM3) * S.lv.scale[level])
    far = lambda uu, vv, zz=z: S.world_of(d, uu, vv, zz)[0]
    if kind == "z_neg":
        return S, d, p, "xw", 2, float(rec["xw"][2]), float(far(u, v, -1.0)[2]), "z_neg"
    if kind in ("u_min", "u_max"):
        S.points[p] = S.points[S.point(d, 20.0 if kind == "u_min" else 1221.0, v, z, level)]; S.near(d, p, 0.0, 0.0, 10, level, 20.0 if kind == "u_min" else 1221.0, v)
        return S, d, p, "xw", 0, float(S.points[p]["xw"][0]), float(far(-20.0 if kind == "u_min" else 1261.0, v)[0]), "u_below_min" if kind == "u_min" else "u_at_max"
    if kind in ("v_min", "v_max"):
        S.points[p] = S.points[S.point(d, u, 20.0 if kind == "v_min" else 356.0, z, level)]; S.near(d, p, 0.0, 0.0, 10, level, u, 20.0 if kind == "v_min" else 356.0)
        return S, d, p, "xw", 1, float(S.points[p]["xw"][1]), float(far(u, -20.0 if kind == "v_min" else 396.0)[1]), "v_below_min" if kind == "v_min" else "v_at_max"
    if kind == "dist_min":
        dist = float(np.linalg.norm(far(u, v) * 0 + np.array([(u - float(CAM["cx"])) / float(CAM["fx"]) * z, (v - float(CAM["cy"])) / float(CAM["fy"]) * z, z])))
        return S, d, p, "min_distance", None, dist / 2.0, dist * 2.0, "dist_below"
    if kind == "dist_max":
        dist = float(np.linalg.norm(np.array([(u - float(CAM["cx"])) / float(CAM["fx"]) * z, (v - float(CAM["cy"])) / float(CAM["fy"]) * z, z])))
        return S, d, p, "max_distance", None, dist / 1.1, dist / 1.3, "dist_above"
    if kind == "window_x":
        return S, d, p, "xw", 0, float(rec["xw"][0]), float(far(u + 2 * r, v)[0]), "empty"
    return S, d, p, "xw", 1, float(rec["xw"][1]), float(far(u, v + 2 * r)[1]), "empty"


def _set_field(rec, field, idx, val):
    if idx is None:
        rec[field] = val
    else:
        rec[field][idx] = val


def search_scan_scene(kind, contract="off"):
    """SEARCH_SCAN_GEOMETRIES pairs, each with SEARCH_SCAN_POINTS source points whose one field runs over consecutive f32 values around
    the place where the named bound decides, found by bisection with the oracle.  -> (scene, per pair: (direction, source features))."""
    kfs, points, pdesc, pairs, rows = [], [], [], [], []
    for g in range(SEARCH_SCAN_GEOMETRIES):
        S, d, p, field, idx, a, b, branch = _scan_setup(kind, g)
        probe = S.source(d, p)
        code = S3_BRANCHES.index(branch)

        def second(val):
            _set_field(S.points[p], field, idx, val)
            one = S.build("probe")
            return int(cpu_search(one, contract)[0][0][4 + d][probe]) == code
        lo, hi = F32(a), F32(b)
        assert not second(lo) and second(hi), (kind, g)
        while True:
            mid = F32((np.float64(lo) + np.float64(hi)) / 2)
            if mid == lo or mid == hi:
                break
            if second(mid):
                hi = mid
            else:
                lo = mid
        toward_lo = F32(-np.inf) if lo < hi else F32(np.inf)
        vals = [lo]
        for _ in range(SEARCH_SCAN_POINTS // 2 - 1):
            vals.insert(0, np.nextafter(vals[0], toward_lo, dtype=F32))
        x = hi
        for _ in range(SEARCH_SCAN_POINTS // 2):
            vals.append(x); x = np.nextafter(x, -toward_lo, dtype=F32)
        _set_field(S.points[p], field, idx, vals[0])
        feats = [probe]
        for x in vals[1:]:
            rec = S.points[p].copy(); _set_field(rec, field, idx, x)
            S.points.append(rec); S.pdesc.append(S.pdesc[p])
            feats.append(S.source(d, len(S.points) - 1))
        one = S.build("scan")
        base = len(points)
        pr = one["pairs"][0]
        pr["p1"] = np.where(pr["p1"] >= 0, pr["p1"] + base, -1).astype(np.int32); pr["p2"] = np.where(pr["p2"] >= 0, pr["p2"] + base, -1).astype(np.int32)
        pr["k1"], pr["k2"] = 2 * g, 2 * g + 1
        kfs += one["kfs"]; points += list(one["points"]); pdesc += list(one["pdesc"]); pairs.append(pr); rows.append((d, feats, code))
    pts = np.array(points, MP_DTYPE)
    return dict(name="scan_" + kind, kfs=kfs, points=pts, pdesc=np.array(pdesc, np.uint8).reshape(len(pts), 32), pairs=pairs, th=TH_SIM3, expect={}), rows


def random_search_scene(seed, n_points=300, n_pairs=1, noise=0.7, share_matched=0.3, slots=None):
    """n_pairs independent pairs of keyframes that see one random cloud each: every physical point has a map point in either map, features
    at its two images (pixel noise), descriptors a few bits from a common one; a share of KF1's features arrives already matched."""
    rng = np.random.default_rng([555, seed, n_points, n_pairs])
    kfs, points, pdesc, pairs = [], [], [], []
    for q in range(n_pairs):
        if slots is not None and q > 0:                          # the first pair's keyframes again, other tables: a share of the
            pr = dict(pairs[0])                                  # points NULL, the already-matched entries redrawn
            pr["p1"] = np.where(rng.random(len(pr["p1"])) < 0.2, -1, pr["p1"]).astype(np.int32)
            pr["p2"] = np.where(rng.random(len(pr["p2"])) < 0.2, -1, pr["p2"]).astype(np.int32)
            m = np.full(len(pr["p1"]), -1, np.int32)
            hit = rng.random(len(m)) < share_matched
            m[hit] = rng.integers(-2, len(pr["p2"]) + 3, int(hit.sum()))
            m[m == -1] = -2
            m[~hit] = -1
            pr["matched12"] = m
            pairs.append(pr)
            continue
        S = Sim3Scene(1000 + 17 * seed + q, s12=float(rng.uniform(0.7, 1.5)), rot=rng.normal(0, 0.02, 3), t12=rng.normal(0, 0.2, 3))
        S.rng = rng
        f1, f2 = [], []
        for j in range(n_points):
            u2, v2, z2 = float(rng.uniform(-30, 1270)), float(rng.uniform(-20, 395)), float(rng.uniform(4, 30))
            X1w, _ = S.world_of(0, u2, v2, z2)
            x1c = X1w @ S.T[0][:3, :3].T + S.T[0][:3, 3]
            if x1c[2] < 0.5:
                continue
            u1, v1 = float(CAM["fx"]) * x1c[0] / x1c[2] + float(CAM["cx"]), float(CAM["fy"]) * x1c[1] / x1c[2] + float(CAM["cy"])
            lvl = int(rng.integers(0, 8)); base = fc.rand_desc(rng)
            P1 = S.point(0, u2, v2, z2, lvl, desc=fc.flipped(base, int(rng.integers(0, 30)), rng)) if rng.random() < 0.9 else -1
            P2 = S.point(1, u1, v1, float(x1c[2]), lvl, desc=fc.flipped(base, int(rng.integers(0, 30)), rng)) if rng.random() < 0.9 else -1
            octs = [int(np.clip(lvl + rng.integers(-2, 2), 0, 7)) for _ in range(2)]
            if -60 < u1 < 1300 and -60 < v1 < 440:
                f1.append(S.feature(0, u1 + rng.normal(0, noise), v1 + rng.normal(0, noise), fc.flipped(base, int(rng.integers(0, 60)), rng), octs[0], P1))
                f2.append(S.feature(1, u2 + rng.normal(0, noise), v2 + rng.normal(0, noise), fc.flipped(base, int(rng.integers(0, 60)), rng), octs[1], P2))
        for a, b in zip(f1, f2):
            if rng.random() < share_matched:
                S.matched[a] = b if rng.random() < 0.8 else int(rng.choice([-2, 100000]))
        one = S.build("r")
        base_p = len(points)
        pr = one["pairs"][0]
        pr["p1"] = np.where(pr["p1"] >= 0, pr["p1"] + base_p, -1).astype(np.int32); pr["p2"] = np.where(pr["p2"] >= 0, pr["p2"] + base_p, -1).astype(np.int32)
        if slots is None:
            pr["k1"], pr["k2"] = 2 * q, 2 * q + 1
            kfs += one["kfs"]
        else:                                                    # every pair on the same two slots (the first pair's keyframes)
            pr["k1"], pr["k2"] = 0, 1
            if q == 0:
                kfs += one["kfs"]
        points += list(one["points"]); pdesc += list(one["pdesc"]); pairs.append(pr)
    pts = np.array(points, MP_DTYPE)
    return dict(name="random_search_%d" % seed, kfs=kfs, points=pts, pdesc=np.array(pdesc, np.uint8).reshape(len(pts), 32), pairs=pairs,
                th=TH_SIM3, expect={})
