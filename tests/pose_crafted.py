"""Crafted PoseOptimization problems, shared by test_pose_crafted.py (the CPU oracle takes the path each case exists for) and
test_gpu_pose_crafted.py (the kernel agrees with the oracle on them).  CASES is a named table like ba_cases.CASES; a case is a dict:

  edges, cam, T0   the problem: pose_cases.EDGE_DTYPE records, a camera dict, the prior (4, 4) f32
  expect           (optional) what the outcome is BY CONSTRUCTION, never taken from the oracle:
                     flags (n,) u8, n_good, and either `T_bytes` (the returned pose, byte for byte) or `T_close` (the true pose, to
                     be met within pose_cases.pose_close(..., 1e-5))
  paths            the path-report entries (pose_cases.optimize_paths) the case exists for, see paths_missing()
  no_move          the oracle returns the prior's bytes: the kernel has to match byte for byte
  on_threshold     the case sits on a chi2 threshold on purpose and does not move: exempt from the margin condition

Every other case keeps every classified chi2 at least MARGIN (relative) away from its threshold: the kernel and the oracle sum in
different orders (about 1e-13 relative), so a flag cannot differ for that reason.  A seeded case that fails this gets another seed.

Exact cases follow test_pose_oracle._exact_problem: fx = fy = 512, bf = 256, dyadic points at depths 4 / 8 / 16, inv_sigma2 = 1, so
every projection is exact in f32 and the optimum is the true pose itself."""
import numpy as np

import pose_cases as pc

F32 = np.float32
MARGIN = 1e-6
EXACT_CAM = dict(fx=F32(512), fy=F32(512), cx=F32(320), cy=F32(240), mbf=F32(256))
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)
SIZES = (3, 9, 10, 63, 64, 65, 255, 256, 257, 512, 513)

# the priors with an exact quaternion: identity (tr > 0) and the three half turns (tr = -1: one `tr <= 0` branch each)
EXACT_PRIORS = {"identity": np.diag([1.0, 1.0, 1.0]), "half_x": np.diag([1.0, -1.0, -1.0]), "half_y": np.diag([-1.0, 1.0, -1.0]),
                "half_z": np.diag([-1.0, -1.0, 1.0])}
EXACT_QUAT = {"identity": "tr>0", "half_x": "i=0", "half_y": "i=1", "half_z": "i=2"}
EXACT_T = np.array([0.25, -0.5, 1.0])


def exact_edges(n, kind, R, t=EXACT_T, seed=3):
    """n observations that are exact in f32 at the pose (R, t), R a signed permutation; x >= -2 keeps every uR >= 0."""
    rng = np.random.default_rng(seed)
    Z = rng.choice([4.0, 8.0, 16.0], n)
    X = rng.integers(-32, 64, n) / 16.0; Y = rng.integers(-32, 32, n) / 16.0
    Xc = np.stack([X, Y, Z], 1)
    Xw = (Xc - t) @ R
    e = np.zeros(n, pc.EDGE_DTYPE)
    e["xw"] = Xw
    e["u"] = 512 * X / Z + 320; e["v"] = 512 * Y / Z + 240
    stereo = np.ones(n, bool) if kind == "stereo" else (np.zeros(n, bool) if kind == "mono" else np.arange(n) % 2 == 0)
    e["ur"] = np.where(stereo, e["u"] - 256 / Z, -1.0)
    e["inv_sigma2"] = 1.0
    e["kp_index"] = np.arange(n)
    assert np.array_equal(e["xw"].astype(np.float64), Xw) and np.all(e["ur"][stereo] >= 0)
    return e


def _case(name, edges, cam, T0, expect=None, paths=None, no_move=False, on_threshold=False):
    edges = edges.copy(); edges["kp_index"] = np.arange(len(edges))
    return dict(name=name, edges=edges, cam=cam, T0=np.asarray(T0, np.float64).astype(F32), expect=expect, paths=paths or {},
                no_move=no_move, on_threshold=on_threshold)


def _stays(T0, n, flags=None):
    """The expectation of a problem that does not move: the prior's bytes, the given flags."""
    flags = np.zeros(n, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    return dict(flags=flags, n_good=int(n - flags.sum()), T_bytes=np.asarray(T0, np.float64).astype(F32).tobytes())


# ---------------------------------------------------------------- exact at the truth
def exact_cases():
    out = []
    for pname, R in EXACT_PRIORS.items():
        T0 = pc.pose(R, EXACT_T)
        for kind in ("mono", "stereo", "mixed"):
            e = exact_edges(40, kind, R)
            out.append(_case("exact_%s_%s" % (pname, kind), e, EXACT_CAM, T0, expect=_stays(T0, 40),
                             paths=dict(quat=EXACT_QUAT[pname], endings_all="rho==0", small_exp_min=4), no_move=True))
    return out


# ---------------------------------------------------------------- threshold probes
def between_weight(thr, err=1.5):
    """An f32 weight w whose chi2 = err * (w * err) (exact in f64) lies strictly between the f32 threshold and the next f32 above it and
    rounds DOWN to the threshold: an inlier by the reference's f32 compare, an outlier by a compare in f64."""
    nxt = np.nextafter(thr, F32(np.inf))
    w0 = F32(np.float64(thr) / (err * err))
    for step in range(-64, 65):
        w = (w0.view(np.int32) + np.int32(step)).view(F32)
        c = np.float64(err) * (np.float64(w) * np.float64(err))
        if np.float64(thr) < c < np.float64(nxt) and F32(c) == thr:
            return w
    raise AssertionError("no weight between %r and %r" % (thr, nxt))


def probe_pairs(R, seed):
    """Pairs of edges that share one point and observe it at u = proj + d and u = proj - d with the same weight: their gradients cancel
    exactly, so the pose does not move, and their chi2 is d * (w * d) exactly.  -> (edges, expected flags)"""
    rng = np.random.default_rng(seed)
    up = lambda x: np.nextafter(x, F32(np.inf))
    rows = [("mono", CHI2_MONO, 1.0), ("mono", up(CHI2_MONO), 1.0), ("stereo", CHI2_STEREO, 1.0), ("stereo", up(CHI2_STEREO), 1.0),
            ("mono", between_weight(CHI2_MONO), 1.5)]
    edges, flags = [], []
    for kind, w, d in rows:
        Z = float(rng.choice([4.0, 8.0, 16.0])); X = int(rng.integers(-16, 64)) / 16.0; Y = int(rng.integers(-32, 32)) / 16.0
        u = 512 * X / Z + 320
        for sign in (1.0, -1.0):
            e = np.zeros((), pc.EDGE_DTYPE)
            e["xw"] = (np.array([X, Y, Z]) - EXACT_T) @ R
            e["u"] = u + sign * d; e["v"] = 512 * Y / Z + 240
            e["ur"] = u - 256 / Z if kind == "stereo" else -1.0             # the uR residual stays 0
            e["inv_sigma2"] = w
            assert float(e["u"]) == u + sign * d and (kind == "mono" or float(e["ur"]) >= 0)
            edges.append(e)
            chi2 = F32(np.float64(d) * (np.float64(w) * np.float64(d)))     # the reference's (float)chi2
            flags.append(int(chi2 > (CHI2_MONO if kind == "mono" else CHI2_STEREO)))
    return np.array(edges, pc.EDGE_DTYPE), np.array(flags, np.uint8)


def probe_cases():
    out = []
    for k, (pname, R) in enumerate(EXACT_PRIORS.items()):
        T0 = pc.pose(R, EXACT_T)
        pe, pf = probe_pairs(R, 20 + k)
        assert pf.tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0]
        e = np.concatenate([exact_edges(15, "mixed", R, seed=40 + k), pe, exact_edges(15, "mixed", R, seed=60 + k)])
        flags = np.concatenate([np.zeros(15, np.uint8), pf, np.zeros(15, np.uint8)])
        out.append(_case("probe_" + pname, e, EXACT_CAM, T0, expect=_stays(T0, len(e), flags),
                         paths=dict(quat=EXACT_QUAT[pname], endings_all="rho==0", margin_max=1e-7), no_move=True, on_threshold=True))
    return out


# ---------------------------------------------------------------- half-turn and far priors that move
# a wrong sign in the i = 2 branch turns a roll about the optical axis z into the opposite roll, and the solver finds its way back from
# there: the tilted axis is what notices it
AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0), "111": (1.0, 1.0, 1.0), "ztilt": (0.6, 0.4, 1.0)}


# what the prior of some of these (truth turned by 1 deg) does in Quaterniond(Matrix3d) / normalizeRotation
FAR_PATHS = {"far_x_179p9": dict(quat="i=0", w_flip=True), "far_111_180": dict(quat="i=1", w_flip=True), "far_z_180": dict(quat="i=2", w_flip=True),
             "far_y_180": dict(quat="i=1", w_flip=False), "far_z_m179p9": dict(quat="i=2", w_flip=False),
             "far_ztilt_119p99": dict(quat="i=2", w_flip=False)}


def far_cases():
    out = []
    for kd, deg in enumerate((179.9, 180.0, -179.9, 119.99, 120.01)):
        for ka, (aname, axis) in enumerate(AXES.items()):
            rng = np.random.default_rng(300 + 10 * kd + ka)
            a = np.array(axis) / np.linalg.norm(axis)
            T = pc.pose(pc.rodrigues(a * np.deg2rad(deg)), rng.normal(size=3) * 2.0)
            e, _, _ = pc.make_problem(rng, 30, "mixed", 0.0, noise=0.0, T=T)
            T0 = pc.perturb(T, rng, 1.0, 0.02)
            name = "far_%s_%s" % (aname, ("%g" % deg).replace("-", "m").replace(".", "p"))
            expect = dict(flags=np.zeros(30, np.uint8), n_good=30, T_close=T)
            out.append(_case(name, e, pc.CAM, T0, expect=expect, paths=dict(moves=True, **FAR_PATHS.get(name, {}))))
            if abs(deg) < 170 and aname != "111":          # the prior's rotation IS the truth's: tr on the side of 0 the angle says
                out.append(_case(name + "_shifted", e, pc.CAM, pc.perturb(T, rng, 0.0, 0.02), expect=expect,
                                 paths=dict(moves=True, quat="tr>0" if deg < 120 else "i=%d" % {"x": 0, "y": 1, "z": 2, "ztilt": 2}[aname], w_flip=False)))
    # a prior whose f32 rotation is visibly non-orthonormal: entries rounded to 1e-3
    rng = np.random.default_rng(399)
    T = pc.pose(pc.rodrigues(np.array([0.6, -0.64, 0.48]) * np.deg2rad(175.0)), rng.normal(size=3) * 2.0)
    e, _, _ = pc.make_problem(rng, 30, "mixed", 0.0, noise=0.0, T=T)
    T0 = pc.perturb(T, rng, 1.0, 0.02)
    T0[:3, :3] = np.round(T0[:3, :3], 3)
    assert np.abs(T0[:3, :3] @ T0[:3, :3].T - np.eye(3)).max() > 2e-4
    out.append(_case("far_rounded_prior", e, pc.CAM, T0, expect=dict(flags=np.zeros(30, np.uint8), n_good=30, T_close=T),
                     paths=dict(moves=True)))
    return out


# ---------------------------------------------------------------- solver exits: seeded noisy problems chosen by the path report
# (name, arguments of _noisy, the paths it was chosen for).  The search walked default_rng(seed) from seed 0 (n = 12, 40, 70) and from
# seed 10 (n = 70) upwards, 30 % gross outliers, 1 px noise, a prior 2 deg / 5 cm off, and took the first seed that takes the path and
# keeps the margin.
EXITS = [
    ("nstop", dict(seed=0, n=12), dict(endings_all="nStop>=3")),
    ("qmax_rejected_trial", dict(seed=0, n=40), dict(endings_all="qmax==10", last_rejected=True)),
    ("ten_iterations", dict(seed=2, n=12), dict(endings_any="ten_iterations", reentered_min=1)),
    ("reentry", dict(seed=10, n=70), dict(reentered_min=2, nbad_drops=True, last_rejected=True)),
    ("last_round_change", dict(seed=12, n=70), dict(last_round_changes_min=1, reentered_min=1)),
    ("rho_zero_noisy", dict(seed=14, n=70), dict(endings_any="rho==0", last_rejected=True)),
    # every edge moved by 150 px or more and the prior at the truth: all outliers after round 0, rounds 1 - 3 have no active edge
    ("all_outliers", dict(seed=8, n=30, ratio=1.0, noise=0.0, deg=0.0, metres=0.0, gross=150.0), dict(endings_any="no_active_edge")),
]


def _noisy(seed, n, ratio=0.3, noise=1.0, deg=2.0, metres=0.05, gross=20.0, kind="mixed"):
    rng = np.random.default_rng(seed)
    e, T, _ = pc.make_problem(rng, n, kind, ratio, noise=noise, gross=gross)
    return e, pc.perturb(T, rng, deg, metres)


def exit_cases():
    out = []
    for name, args, paths in EXITS:
        e, T0 = _noisy(**args)
        out.append(_case("exit_" + name, e, pc.CAM, T0, paths=paths))
    return out


# ---------------------------------------------------------------- sizes around the 256-thread stride and the 64-lane butterfly
SIZE_SEEDS = {}           # n -> seed, for an n at which seed 700 + n fails the margin condition (none does)


def size_cases():
    out = []
    for n in SIZES:
        pname = list(EXACT_PRIORS)[n % 4]
        R = EXACT_PRIORS[pname]
        T0 = pc.pose(R, EXACT_T)
        e = exact_edges(n, "mixed", R, seed=500 + n)
        out.append(_case("size_%d_exact" % n, e, EXACT_CAM, T0, expect=_stays(T0, n),
                         paths=dict(endings_all="rho==0", rounds=1 if n < 10 else 4), no_move=True))
        for which, idx in (("first", 0), ("last", n - 1)):
            g = e.copy()
            g["u"][idx] += F32(64.0)                        # chi2 = 4096 at the truth
            flags = np.zeros(n, np.uint8); flags[idx] = 1
            # from 10 edges on the rounds after the first run without the outlier and restart at the prior, which is the truth: no move
            out.append(_case("size_%d_%s_out" % (n, which), g, EXACT_CAM, T0, expect=_stays(T0, n, flags) if n >= 10 else None,
                             paths=dict(rounds=1 if n < 10 else 4), no_move=n >= 10))
        e, T0 = _noisy(SIZE_SEEDS.get(n, 700 + n), n, 0.2)
        out.append(_case("size_%d_noisy" % n, e, pc.CAM, T0, paths=dict(moves=True)))
    return out


# ---------------------------------------------------------------- depth
def depth_cases():
    out = []
    R = EXACT_PRIORS["identity"]
    T = pc.pose(R, EXACT_T)
    # a point 4 m BEHIND the camera at the truth, observed 50 px from where the projection formula puts it
    for kind in ("mono", "stereo"):
        e = exact_edges(31, kind, R, seed=80)
        Xc = np.array([1.5, -0.75, -4.0])
        e["xw"][13] = (Xc - EXACT_T) @ R
        e["u"][13] = 512 * Xc[0] / Xc[2] + 320 + 50; e["v"][13] = 512 * Xc[1] / Xc[2] + 240
        if kind == "stereo":
            e["ur"][13] = 320.0                             # any uR >= 0 keeps the edge a stereo edge
        flags = np.zeros(31, np.uint8); flags[13] = 1
        T0 = pc.perturb(T, np.random.default_rng(81), 1.0, 0.02)
        out.append(_case("depth_behind_" + kind, e, EXACT_CAM, T0, expect=dict(flags=flags, n_good=30, T_close=T), paths=dict(moves=True)))
    # a point ON the camera plane at the prior: p2 == 0.  mono with x != 0: the error is infinite; stereo with x == 0: it is NaN at once.
    # Every sum turns NaN, every trial is rejected, NaN > thr is false: all flags 0 and the prior comes back (the reference's behaviour,
    # DESIGN.md Q24b).
    for kind, x in (("mono", 1.5), ("stereo", 0.0)):
        e = exact_edges(30, kind, R, seed=82)
        e["xw"][7] = (np.array([x, 0.5, 0.0]) - EXACT_T) @ R
        out.append(_case("depth_zero_" + kind, e, EXACT_CAM, T, expect=_stays(T, 30), paths=dict(non_finite=True, endings_all="ten_iterations", rejected_all=10),
                         no_move=True))
    return out


# ---------------------------------------------------------------- k_pose_edges: matched key points of an uploaded frame pair
FRAME_SIZES = (255, 256, 257, 513)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def match_pattern(N, n_last):
    """match (N,) int32 of a Current frame with N key points: matches at 0, 63, 64, 255, 256 and N - 1 (the ballot's lane, wave and
    256-stride edges), a run of 64 set and a run of 64 unset that both cross a wave boundary, every third key point beyond 260, and two
    key points (0 and 63) matched to the same point."""
    m = np.full(N, -1, np.int32)
    idx = sorted(set(i for i in (0, 63, 64, 255, 256, N - 1) if i < N) | set(range(96, 160)) | set(range(260, N, 3)))
    assert not set(range(160, 224)) & set(idx)
    for i in idx:
        m[i] = (i * 37 + 11) % n_last
    m[63] = m[0]
    return m


def edge_frames(N, seed, inv_sigma2):
    """A Last frame with N map points and a Current frame with N key points that observe the points match_pattern() assigns them from
    the true pose (1 px noise times the level's scale): every octave including the top one, uRight < 0, == 0 and > 0 in turn.
    -> dict(cur, last, xw, flags, match, T0 (the prior, 1 deg / 2 cm off), cam, edges (what k_pose_edges has to build, in key-point
    order))."""
    rng = np.random.default_rng(seed)
    cam = pc.CAM
    fx, fy, cx, cy, bf = [float(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf")]
    pts, T, _ = pc.make_problem(rng, N, "stereo", 0.0, noise=0.0)
    xw = pts["xw"].copy()
    match = match_pattern(N, N)
    nlev = len(inv_sigma2)

    def frame(n):
        k = np.zeros(n, KP_DTYPE)
        k["x"] = rng.uniform(20, 1200, n); k["y"] = rng.uniform(20, 350, n); k["size"] = 31.0; k["response"] = 50.0; k["class_id"] = -1
        k["octave"] = np.arange(n) % nlev
        return dict(kp=k, desc=rng.integers(0, 256, (n, 32)).astype(np.uint8), ur=np.full(n, -1.0, F32), depth=np.full(n, -1.0, F32),
                    Tcw=np.eye(4, dtype=F32))
    cur, last = frame(N), frame(N)
    i = np.nonzero(match >= 0)[0]
    Xc = xw[match[i]].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    s = 1.2 ** cur["kp"]["octave"][i]
    u = fx * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(size=len(i)) * s
    cur["kp"]["x"][i] = u
    cur["kp"]["y"][i] = fy * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(size=len(i)) * s
    cur["ur"][:] = np.where(np.arange(N) % 3 == 0, -1.0, 0.0)
    ur = u - bf / Xc[:, 2] + rng.normal(size=len(i)) * s
    third = (i % 3 == 2) & (ur > 0)
    cur["ur"][i[third]] = ur[third]
    assert third.sum() >= 10
    e = np.zeros(len(i), pc.EDGE_DTYPE)
    e["xw"] = xw[match[i]]; e["u"] = cur["kp"]["x"][i]; e["v"] = cur["kp"]["y"][i]; e["ur"] = cur["ur"][i]
    e["inv_sigma2"] = np.asarray(inv_sigma2, F32)[cur["kp"]["octave"][i]]; e["kp_index"] = i
    return dict(cur=cur, last=last, xw=xw, flags=np.ones(N, np.uint8), match=match, T0=pc.perturb(T, rng, 1.0, 0.02).astype(F32), cam=cam,
                edges=e)


def inv_level_sigma2(scale_factor=1.2, nlevels=8):
    """mvInvLevelSigma2 as ORBextractor's constructor computes it (ORBextractor.cc:419-430)."""
    s = np.zeros(nlevels, F32); s[0] = 1
    for k in range(1, nlevels):
        s[k] = F32(np.float64(s[k - 1]) * np.float64(F32(scale_factor)))
    return (F32(1.0) / (s * s)).astype(F32)


def build_cases():
    cases = exact_cases() + probe_cases() + far_cases() + exit_cases() + size_cases() + depth_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in cases}


_cases = None
_oracle_results = {}


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
    return _cases


def names():
    return list(cases())


def oracle_result(name):
    """(return value, Tcw, flags, stats, paths) of the oracle on a case; computed once, shared, not to be modified."""
    if name not in _oracle_results:
        c = cases()[name]
        r = pc.optimize_paths(c["edges"], c["cam"], c["T0"])
        for a in r[1:4]:
            a.setflags(write=False)
        _oracle_results[name] = r
    return _oracle_results[name]


def paths_missing(case, result):
    """The entries of case["paths"] the oracle's run did NOT take (empty = the case does what it exists for)."""
    r, T, flags, st, rep = result
    want, miss = case["paths"], []
    rounds = int(st[0])
    nbad = [int(st[3 + 3 * k]) for k in range(rounds)]
    checks = {
        "quat": lambda v: rep["quat"] == v,
        "w_flip": lambda v: rep["w_flip"] == v,
        "small_exp_min": lambda v: rep["small_exp"] >= v,
        "non_finite": lambda v: rep["non_finite"] == v,
        "endings_all": lambda v: rounds > 0 and all(x == v for x in rep["endings"]),
        "endings_any": lambda v: v in rep["endings"],
        "rejected_all": lambda v: rounds > 0 and all(x == v for x in rep["rejected"]),
        "last_rejected": lambda v: any(int(st[2 + 3 * k]) for k in range(rounds)) == v,
        "reentered_min": lambda v: rep["reentered"] >= v,
        "nbad_drops": lambda v: any(b < a for a, b in zip(nbad, nbad[1:])) == v,
        "last_round_changes_min": lambda v: rep["last_round_changes"] >= v,
        "margin_max": lambda v: rep["margin"] <= v,
        "rounds": lambda v: rounds == v,
        "moves": lambda v: (T.tobytes() != case["T0"].tobytes()) == v,
    }
    for k, v in want.items():
        if not checks[k](v):
            miss.append((k, v))
    return miss
