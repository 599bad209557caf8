"""Shared by test_ba_oracle.py, test_gpu_ba.py, tools/fuzz_ba.py and tools/bench_ba.py: the Optimizer::LocalBundleAdjustment CPU oracle
(tests/cpp/ba_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory) and seeded crafted scenes in plain numpy.

A problem is dict(kfs (KF_DTYPE; the first n_local are the local keyframes), n_local, xw (P, 3) f32, edges (EDGE_DTYPE, insertion
order), ref_kf (P,) i32) -- what frontend.local_bundle_adjustment takes.  A scene adds the ground truth (gt_T (K, 4, 4), gt_xw) and
`planted` (edge indices of the planted outliers).  Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KF_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("fixed", "u1"),
                     ("pad", "u1", (3,))])                                                             # sd_ba_keyframe, 88 bytes
EDGE_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"), ("tag", "<i4"),
                       ("reserved", "<i4")])                                                           # sd_ba_edge, 32 bytes
STATS_DTYPE = np.dtype([("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("rejected", "<i4", (2,)), ("n_level1", "<i4"),
                        ("n_erased", "<i4"), ("chi2", "<f8", (2,))])                                   # sd_ba_stats, 48 bytes
BRANCHES = ["mono_edge", "stereo_edge", "fixed_local", "edge_to_fixed", "single_mono", "level1_chi2", "level1_depth", "point_inactive",
            "kf_inactive", "rejected", "stop_nbad", "stop_terminate", "noop", "huber", "pose_pose", "factor_fail", "erase_chi2",
            "erase_depth", "round2_empty", "fixed_plus_one_local", "no_pose", "duplicate_edge", "last_rejected_r1", "last_rejected_r2",
            "level1_point_active", "stereo_between", "quat_tr", "quat_i0", "quat_i1", "quat_i2"]
# flags of the oracle: the deliberately wrong twins (T_* of ba_oracle.cpp); tests/ba_crafted.py names the case each must differ on
TWINS = dict(f32_compare=1, no_depth_test=2, fresh_chi2=4, level1_active=8, lambda_carried=16, delta_swapped=32)
MARGINS = ["chi2", "depth", "rho", "stop"]
MARGIN = 1e-6
CHOL_TILE = 48          # SD_BA_NB of k_ba.h: rows of the reduced camera system factorised per LDS tile
THREADS = 256           # SD_BA_THREADS
CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, mbf=40.0)

_oracles = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="ba_oracle_")
        so = os.path.join(d, "libba_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []          # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "ba_oracle.cpp")])
        L = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        L.sd_ba_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_ba_oracle_round1_points.argtypes = [vp, i]
        L.sd_ba_oracle.argtypes = [i, i, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp]
        assert L.sd_ba_oracle_branch_count() == len(BRANCHES)
        _oracles[contract] = L
    return _oracles[contract]


def branches(L, reset=False):
    b = L.sd_ba_oracle_branches()
    out = {name: int(b[i]) for i, name in enumerate(BRANCHES)}
    if reset:
        L.sd_ba_oracle_reset_branches()
    return out


def problem_of(scene):
    return {k: scene[k] for k in ("kfs", "n_local", "xw", "edges", "ref_kf")}


def run_oracle(prob, contract="off", reverse=False, twin=None):
    """One problem through the oracle.  reverse = the same edges in reversed insertion order (per-edge outputs come back in the
    caller's order).  twin = a name of TWINS: the deliberately wrong variant.  Returns dict(Tcw (n_local, 4, 4), xw, normal, dist,
    level1, erase, stats (STATS_DTYPE scalar), margins {name: v}, branches {name: count}, round1_xw, cached (2, E): every edge's cached
    chi2 as the first and the second classification read it).  Nothing of `prob` is modified."""
    L = oracle(contract)
    kfs = np.ascontiguousarray(prob["kfs"], KF_DTYPE); xw = np.ascontiguousarray(prob["xw"], F32).reshape(-1, 3)
    e = np.ascontiguousarray(prob["edges"], EDGE_DTYPE); ref = np.ascontiguousarray(prob["ref_kf"], np.int32)
    if reverse:
        e = np.ascontiguousarray(e[::-1])
    nl, nk, npt, ne = int(prob["n_local"]), len(kfs), len(xw), len(e)
    T = np.zeros((max(nl, 1), 16), F32); xo = np.zeros((max(npt, 1), 3), F32); nrm = np.zeros((max(npt, 1), 3), F32)
    dist = np.zeros(max(npt, 1), F32); l1 = np.zeros(max(ne, 1), np.uint8); er = np.zeros(max(ne, 1), np.uint8)
    st = np.zeros(1, STATS_DTYPE); mg = np.zeros(4, np.float64); cached = np.zeros((2, max(ne, 1)), np.float64)
    branches(L, reset=True)
    rc = L.sd_ba_oracle(nk, nl, _p(kfs), npt, _p(xw), ne, _p(e), _p(ref), _p(T), _p(xo), _p(nrm), _p(dist), _p(l1), _p(er), _p(st), _p(mg),
                        TWINS[twin] if twin else 0, _p(cached))
    assert rc == 0, rc
    r1 = np.zeros(max(3 * npt, 1), np.float64)
    r1 = r1[:L.sd_ba_oracle_round1_points(_p(r1), 3 * npt)].reshape(-1, 3)
    l1, er, cached = l1[:ne], er[:ne], cached[:, :ne]
    if reverse:
        l1, er, cached = l1[::-1].copy(), er[::-1].copy(), cached[:, ::-1].copy()
    return dict(Tcw=T[:nl].reshape(nl, 4, 4), xw=xo[:npt], normal=nrm[:npt], dist=dist[:npt], level1=l1, erase=er, stats=st[0],
                margins=dict(zip(MARGINS, mg.tolist())), branches=branches(L), round1_xw=r1, cached=cached)


def run_oracle_plain(prob):
    """run_oracle without the branch counters (they are process-wide): the form tools/bench_ba.py calls from several threads."""
    r = run_oracle(prob)
    r.pop("branches"); r.pop("round1_xw"); r.pop("cached")
    return r


KINDS = (("pose", "Tcw"), ("points", "xw"), ("normal", "normal"), ("dist", "dist"))
COUNTS = ("iterations", "trials", "rejected", "n_level1", "n_erased")


def spread_of(prob, base):
    """The yardstick of the device tolerance: the largest difference of each kind of output between the oracle as built (`base`) and
    (a) the oracle built with -ffp-contract=fast, (b) the oracle fed the same edges in reversed insertion order.  None when a variant
    takes another decision (the problem is ill-conditioned or sits on a threshold)."""
    out = {kind: 0.0 for kind, _ in KINDS}
    for var in (run_oracle(prob, contract="fast"), run_oracle(prob, reverse=True)):
        if not (np.array_equal(var["erase"], base["erase"]) and np.array_equal(var["level1"], base["level1"])
                and all(np.array_equal(var["stats"][f], base["stats"][f]) for f in COUNTS)):
            return None
        for kind, key in KINDS:
            if base[key].size:
                out[kind] = max(out[kind], float(np.abs(var[key].astype(np.float64) - base[key].astype(np.float64)).max()))
    return out


def mismatch(got, want, spread, log=None):
    """None when a device result equals the oracle's: decisions and counts exactly, values within max(10 x spread, 4 f32 ulps of the
    entry) (DESIGN Q37); else what differs."""
    for f in COUNTS:
        if log:
            log("%s device %s oracle %s" % (f, got["stats"][f], want["stats"][f]))
        if not np.array_equal(got["stats"][f], want["stats"][f]):
            return "%s: device %s, oracle %s" % (f, got["stats"][f], want["stats"][f])
    if not np.array_equal(got["level1"], want["level1"]):
        return "level1 flags differ at %s" % np.flatnonzero(got["level1"] != want["level1"])[:8]
    if not np.array_equal(got["erase"], want["erase"]):
        return "erase flags differ at %s" % np.flatnonzero(got["erase"] != want["erase"])[:8]
    for kind, key in KINDS:
        g, w = got[key].astype(np.float64), want[key].astype(np.float64)
        if g.shape != w.shape:
            return "%s: shape %s vs %s" % (kind, g.shape, w.shape)
        if not g.size:
            continue
        tol = np.maximum(10.0 * spread[kind], 4.0 * np.spacing(np.abs(want[key]).astype(F32)).astype(np.float64))
        if log:
            log("%s: max |device - oracle| %.3g, spread %.3g" % (kind, np.abs(g - w).max(), spread[kind]))
        if not (np.abs(g - w) <= tol).all():
            return "%s: max |device - oracle| %.3g (%.1f x its tolerance)" % (kind, np.abs(g - w).max(), (np.abs(g - w) / tol).max())
    return None


# ---------------------------------------------------------------- scenes
def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R; T[:3, 3] = t
    return T


def make_scene(seed, n_local, n_fixed, n_points, stereo_frac=1.0, noise=0.3, pose_noise=(0.01, 0.03), point_noise=0.03, obs_per_point=None,
               fixed_local=(), mild=0.03, cam=CAM):
    """Keyframes on a gently curving track looking down +z at a cloud 4-10 m ahead; every point is seen by obs_per_point keyframes
    (default: all) drawn per point; edges are inserted point by point, keyframes ascending (the reference's loop with its map ordered by
    table index).  Observations are f32 with Gaussian pixel noise; the start is the ground truth plus (rotation rad, translation m) and
    point noise on the non-fixed vertices.  A fraction `mild` of the edges is shifted by 8-14 px: round 1 sends them to level 1, so
    round 2 solves a different problem and does not start at its own optimum, where the sign of rho would be rounding noise."""
    rng = np.random.default_rng(seed)
    K = n_local + n_fixed
    gt_T = np.zeros((K, 4, 4))
    for k in range(K):
        R = rodrigues(np.array([0.02 * rng.standard_normal(), 0.05 * (k - K / 2) / max(K, 1) * 4 + 0.01 * rng.standard_normal(), 0.01 * rng.standard_normal()]))
        c = np.array([0.25 * k - 0.125 * K, 0.05 * rng.standard_normal(), 0.1 * rng.standard_normal()])
        gt_T[k] = pose(R, -R @ c)
    gt_xw = np.stack([rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(4.0, 10.0, n_points)], 1)
    kfs = np.zeros(K, KF_DTYPE)
    for k in range(K):
        T = gt_T[k].copy()
        if k < n_local and k not in fixed_local:
            dR = rodrigues(pose_noise[0] * rng.standard_normal(3))
            T = pose(dR @ T[:3, :3], dR @ T[:3, 3] + pose_noise[1] * rng.standard_normal(3))
        kfs[k]["Tcw"] = T.astype(F32).reshape(16)
        for key in ("fx", "fy", "cx", "cy", "mbf"):
            kfs[k][key] = cam[key]
        kfs[k]["fixed"] = 1 if k in fixed_local else 0
    gt_T32 = gt_T.copy()
    for k in range(K):                                   # fixed vertices stay where the table puts them: that IS their truth
        if k >= n_local or k in fixed_local:
            gt_T32[k] = kfs[k]["Tcw"].reshape(4, 4).astype(np.float64)
    edges = []
    for p in range(n_points):
        seen = np.arange(K) if obs_per_point is None else np.sort(rng.choice(K, min(obs_per_point, K), replace=False))
        for k in seen:
            pc = gt_T32[k][:3, :3] @ gt_xw[p] + gt_T32[k][:3, 3]
            u = cam["fx"] * pc[0] / pc[2] + cam["cx"] + noise * rng.standard_normal()
            v = cam["fy"] * pc[1] / pc[2] + cam["cy"] + noise * rng.standard_normal()
            stereo = rng.random() < stereo_frac
            ur = u - cam["mbf"] / pc[2] + noise * rng.standard_normal() if stereo else -1.0
            lvl = int(rng.integers(0, 4))
            edges.append((k, p, u, v, ur, 1.0 / (1.2 ** (2 * lvl)), len(edges), 0))
    edges = np.array(edges, EDGE_DTYPE) if edges else np.zeros(0, EDGE_DTYPE)
    xw = (gt_xw + point_noise * rng.standard_normal(gt_xw.shape)).astype(F32)
    ref = np.zeros(n_points, np.int32)
    ref[::7] = -1
    ref[1::3] = K - 1 if K else -1
    s = dict(kfs=kfs, n_local=n_local, xw=xw, edges=edges, ref_kf=ref if K else np.full(n_points, -1, np.int32), gt_T=gt_T32, gt_xw=gt_xw,
             planted=np.zeros(0, np.int64))
    n_mild = int(np.ceil(mild * len(edges)))
    if n_mild:
        idx = rng.choice(len(edges), n_mild, replace=False)
        ang = rng.uniform(0, 2 * np.pi, n_mild)
        plant(s, idx, np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(8, 14, n_mild)[:, None])
    return s


def plant(scene, idx, shift):
    """Gross outliers: shift the observation of the given edges by `shift` pixels."""
    e = scene["edges"]
    idx = np.asarray(idx, np.int64)
    sh = np.broadcast_to(np.asarray(shift, np.float64), (len(idx), 2))
    e["u"][idx] += sh[:, 0].astype(F32)
    e["v"][idx] += sh[:, 1].astype(F32)
    st = e["ur"][idx] >= 0
    e["ur"][idx[st]] += sh[st, 0].astype(F32)
    scene["planted"] = np.union1d(scene["planted"], idx)
    return scene


def drop_edges(scene, keep):
    scene["edges"] = np.ascontiguousarray(scene["edges"][keep])
    return scene


def case_small():
    """1 local + 2 fixed keyframes, 8 points: no pose-pose block (branch: pose_pose == 0)."""
    return make_scene(101, 1, 2, 8)


def case_mixed():
    """3 local + 2 fixed keyframes, 40 points, mono and stereo mixed (branches: mono_edge, stereo_edge, pose_pose)."""
    return make_scene(102, 3, 2, 40, stereo_frac=0.5)


def case_noise_free():
    """Exact f32 observations from a perturbed start: the ground truth comes back."""
    return make_scene(103, 3, 2, 40, stereo_frac=0.6, noise=0.0, mild=0.0)


def case_fixed_local():
    """A local keyframe with fixed = 1 (branch: fixed_local)."""
    return make_scene(104, 3, 2, 30, fixed_local=(0,))


def case_fixed_plus_one_local():
    """Points seen only by fixed keyframes plus one local keyframe (branch: fixed_plus_one_local)."""
    s = make_scene(105, 3, 3, 30, stereo_frac=0.7)
    e = s["edges"]
    keep = ~((e["point"] < 10) & (e["kf"] < 3) & (e["kf"] != (e["point"] % 3)))
    return drop_edges(s, keep)


def case_single_mono():
    """A point with a single monocular edge: its Hll is singular without lambda (branch: single_mono)."""
    s = make_scene(106, 3, 2, 30, stereo_frac=0.7)
    e = s["edges"]
    first = np.flatnonzero(e["point"] == 4)[1]
    keep = (e["point"] != 4) | (np.arange(len(e)) == first)
    s = drop_edges(s, keep)
    i = np.flatnonzero(s["edges"]["point"] == 4)[0]
    s["edges"]["ur"][i] = -1.0
    return s


def case_outliers():
    """Planted gross outliers and an edge of negative depth (branches: level1_chi2, level1_depth, erase_chi2, erase_depth, huber)."""
    s = make_scene(107, 3, 3, 40, stereo_frac=0.6, mild=0.0)
    rng = np.random.default_rng(1107)
    pts = rng.choice(40, 12, replace=False)                # one outlier per point: the other five views hold the point in place
    idx = np.array([rng.choice(np.flatnonzero(s["edges"]["point"] == p)) for p in pts])
    ang = rng.uniform(0, 2 * np.pi, len(idx))
    plant(s, idx, np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(25, 60, len(idx))[:, None])
    # a fixed keyframe that looks the other way sees point 0 behind it
    k = len(s["kfs"]) - 1
    e = s["edges"]
    keep = e["kf"] != k
    s = drop_edges(s, keep)
    s["planted"] = np.array([int(np.flatnonzero(np.flatnonzero(keep) == i)[0]) for i in s["planted"] if keep[i]], np.int64)
    T = s["gt_T"][k].copy()
    T[:3, :3] = rodrigues(np.array([0.0, np.pi, 0.0])) @ T[:3, :3]
    T[:3, 3] = rodrigues(np.array([0.0, np.pi, 0.0])) @ T[:3, 3]
    s["kfs"][k]["Tcw"] = T.astype(F32).reshape(16)
    s["gt_T"][k] = s["kfs"][k]["Tcw"].reshape(4, 4)
    neg = np.array([(k, 0, 300.0, 200.0, -1.0, 1.0, 9999, 0)], EDGE_DTYPE)
    s["edges"] = np.concatenate([s["edges"], neg])
    s["planted"] = np.union1d(s["planted"], [len(s["edges"]) - 1])
    return s


def case_point_all_level1():
    """A point all of whose edges go to level 1: inactive in round 2, it keeps its round-1 value (branch: point_inactive)."""
    s = make_scene(108, 3, 2, 30, obs_per_point=3)
    idx = np.flatnonzero(s["edges"]["point"] == 5)
    return plant(s, idx, [[60.0, -45.0], [-50.0, 55.0], [40.0, 70.0]][:len(idx)])


def case_kf_all_level1():
    """A local keyframe all of whose edges go to level 1 (branch: kf_inactive)."""
    s = make_scene(109, 3, 2, 30, obs_per_point=4)
    idx = np.flatnonzero(s["edges"]["kf"] == 2)
    rng = np.random.default_rng(1109)
    ang = rng.uniform(0, 2 * np.pi, len(idx))
    return plant(s, idx, np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(60, 120, len(idx))[:, None])


def case_far_start():
    """A start far enough off that a trial is rejected (branch: rejected)."""
    return make_scene(301, 3, 2, 40, stereo_frac=0.8, pose_noise=(0.15, 0.6), point_noise=1.0)


def case_at_optimum():
    """A start at the ground truth of noisy observations: three iterations in a row gain less than 0.1 % (branch: stop_nbad)."""
    return make_scene(111, 3, 2, 40, stereo_frac=0.6, noise=0.5, pose_noise=(0.0, 0.0), point_noise=0.0, mild=0.0)


def case_empty_no_edges():
    """Keyframes and points, no edge: a no-op (branch: noop)."""
    s = make_scene(112, 2, 1, 5)
    return drop_edges(s, np.zeros(len(s["edges"]), bool))


def case_empty_no_points():
    """Keyframes only (branch: noop)."""
    return make_scene(113, 2, 1, 0)


def case_empty_nothing():
    """No keyframe, no point, no edge (branch: noop)."""
    return make_scene(114, 0, 0, 0)


def case_all_fixed():
    """Every keyframe fixed: no pose block at all, the points alone are refined (branch: no_pose)."""
    return make_scene(201, 2, 2, 12, fixed_local=(0, 1), stereo_frac=0.3, point_noise=1.0, mild=0.1)


def case_duplicate_edge():
    """Two edges between the same keyframe and point (a local and a fixed keyframe, a stereo and a mono pair): the oracle adds them into one
    Hpl block as g2o does, the device takes the sums over pairs of edges; DESIGN Q32 (branch: duplicate_edge)."""
    s = make_scene(116, 3, 2, 30, stereo_frac=0.6)
    e = s["edges"]
    pick = [int(np.flatnonzero((e["point"] == p) & (e["kf"] == k))[0]) for p, k in ((3, 1), (11, 4), (20, 0))]
    dup = e[pick].copy()
    dup["u"] += F32(0.25); dup["v"] -= F32(0.125)
    dup["ur"][2] = -1.0
    dup["tag"] = 7000 + np.arange(len(dup))
    s["edges"] = np.concatenate([e, dup])
    return s


def case_tile(n_local):
    """6 n_local at the Cholesky tile size - 6 / + 0 / + 6 (n_local = 7, 8, 9) and two tiles and a bit (17)."""
    return make_scene(120 + n_local, n_local, 3, 60, stereo_frac=0.6, obs_per_point=5)


def case_edge_count(n_edges):
    """Edge counts at the workgroup size - 1 / + 0 / + 1: the strided edge loops end on a partial, a full and a one-edge pass."""
    s = make_scene(130, 3, 2, 60, stereo_frac=0.6)
    return drop_edges(s, np.arange(len(s["edges"])) < n_edges)


CASES = {
    "small": (case_small, []),
    "mixed": (case_mixed, ["mono_edge", "stereo_edge", "pose_pose", "edge_to_fixed"]),
    "noise_free": (case_noise_free, []),
    "fixed_local": (case_fixed_local, ["fixed_local"]),
    "fixed_plus_one_local": (case_fixed_plus_one_local, ["fixed_plus_one_local"]),
    "single_mono": (case_single_mono, ["single_mono"]),
    "outliers": (case_outliers, ["level1_chi2", "level1_depth", "erase_chi2", "erase_depth", "huber"]),
    "point_all_level1": (case_point_all_level1, ["point_inactive"]),
    "kf_all_level1": (case_kf_all_level1, ["kf_inactive"]),
    "far_start": (case_far_start, ["rejected"]),
    "at_optimum": (case_at_optimum, ["stop_nbad"]),
    "empty_no_edges": (case_empty_no_edges, ["noop"]),
    "empty_no_points": (case_empty_no_points, ["noop"]),
    "empty_nothing": (case_empty_nothing, ["noop"]),
    "all_fixed": (case_all_fixed, ["no_pose"]),
    "duplicate_edge": (case_duplicate_edge, ["duplicate_edge"]),
    "tile_m6": (lambda: case_tile(CHOL_TILE // 6 - 1), ["pose_pose"]),
    "tile_0": (lambda: case_tile(CHOL_TILE // 6), ["pose_pose"]),
    "tile_p6": (lambda: case_tile(CHOL_TILE // 6 + 1), ["pose_pose"]),
    "tile_2p": (lambda: case_tile(2 * CHOL_TILE // 6 + 1), ["pose_pose"]),
    "edges_m1": (lambda: case_edge_count(THREADS - 1), []),
    "edges_0": (lambda: case_edge_count(THREADS), []),
    "edges_p1": (lambda: case_edge_count(THREADS + 1), []),
}

_scenes, _results = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = CASES[name][0]()
    return _scenes[name]


def expected(name):
    """The oracle's answer for a crafted case, computed once and shared."""
    if name not in _results:
        _results[name] = run_oracle(problem_of(scene(name)))
    return _results[name]


def random_scene(seed):
    """tools/fuzz_ba.py: random sizes, stereo share and start error; pixel noise of 0.8-1.5 px (the sigma the chi2 bounds assume) and up to
    6 % gross outliers.  With less noise round 2 converges to the rounding floor inside its 10 iterations more often, and the sign of rho
    there is noise: such a problem sits inside the decision margin and is skipped by the sweep."""
    rng = np.random.default_rng(seed)
    nl, nf, npt = int(rng.integers(1, 12)), int(rng.integers(2, 6)), int(rng.integers(24, 120))
    s = make_scene(seed, nl, nf, npt, stereo_frac=float(rng.uniform(0.2, 1.0)), noise=float(rng.uniform(0.8, 1.5)),
                   obs_per_point=int(rng.integers(3, nl + nf + 1)), pose_noise=(float(rng.uniform(0, 0.05)), float(rng.uniform(0, 0.2))),
                   point_noise=float(rng.uniform(0, 0.3)), mild=0.0)
    n_out = int(rng.integers(1, max(2, len(s["edges"]) // 15)))
    idx = rng.choice(len(s["edges"]), n_out, replace=False)
    ang = rng.uniform(0, 2 * np.pi, n_out)
    return plant(s, idx, np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(20, 80, n_out)[:, None])
