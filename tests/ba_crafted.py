"""Crafted LocalBundleAdjustment problems, shared by test_ba_crafted.py (the CPU oracle meets what each case is built for, every wrong
twin of the oracle differs on the case named for it) and test_gpu_ba_crafted.py (k_ba.h agrees).  Laid out like pose_crafted.py on top of
ba_cases.py (dtypes, run_oracle, spread_of, mismatch, problem_of, make_scene).

EXACT      outcomes known BY CONSTRUCTION, never taken from the oracle.  The camera is pose_crafted.EXACT_CAM (fx = fy = 512, cx = 320,
           cy = 240, mbf = 256); the keyframes are the identity and the three half turns (one Quaterniond(Matrix3d) branch each) with dyadic
           translations, facing one another across a cloud of dyadic points that every observing keyframe sees at depth 4 / 8 / 16, so every
           projection and every uR is exact in f32 and the start is the optimum: poses and points come back with the input's bytes.  A case
           is dict(scene, level1, erase (expected flags), counts (iterations, trials, rejected per round: the rho == 0 ending, see
           EXACT_COUNTS), chi2 (expected final chi2 of the two rounds, None where the case does not state it)).  All of them sit on
           thresholds on purpose and do not move: they are exempt from the margin rule, as pose_crafted's on_threshold cases are.
           last_trial_rejected, the cached-error case after a rejected trial, is one of them: its docstring says why no seed gives it.
SEARCHED   found by a search over seeds (pick): stale_level1, the cached-error case the oracle reports the branch of and fresh_chi2()
           -- plain numpy f64 from the returned f32 poses and points, no code shared with the oracle -- shows the split of; and
           stereo_between, a stereo edge linearised between the two chi2 bounds, for the twin that swaps the Huber deltas.
SCENES     orders, list lengths and sizes: make_scene scenes, reordered or thinned; device against oracle under ba_cases.mismatch with
           the spread recorded in profiles/ba_crafted_tolerance.json."""
import numpy as np

import ba_cases as bc
from pose_crafted import EXACT_CAM, EXACT_PRIORS

F32 = np.float32
CHI2_MONO, CHI2_STEREO = 5.991, 7.815                    # LocalBundleAdjustment compares e->chi2() with these doubles
QUAT_BRANCH = {"identity": "quat_tr", "half_x": "quat_i0", "half_y": "quat_i1", "half_z": "quat_i2"}
# (orientation, translation): the local keyframes, then the fixed cameras.  Depth is zw + tz under the identity and half_z, tz - zw under
# half_x and half_y; points lie at zw = 4 / 8 / 16 and a keyframe observes those it sees at depth 4 / 8 / 16.
EXACT_LOCAL = [("identity", (0.25, -0.5, 0.0)), ("half_x", (-0.25, 0.5, 12.0)), ("half_y", (0.5, 0.25, 12.0)), ("half_z", (-0.5, -0.25, 0.0))]
EXACT_FIXED = [("identity", (-0.25, 0.25, 8.0)), ("half_x", (0.25, -0.25, 20.0)), ("half_y", (-0.5, 0.5, 20.0)), ("half_z", (0.5, -0.5, 0.0))]
# What the rho == 0 ending gives (DESIGN Q33, Q19-Q22).  At the optimum b = 0, so the solve returns x = 0, the trial's chi2 equals the
# current one and rho = 0 / 1e-3 = 0: `rho > 0` fails, the trial is REJECTED (estimates restored, lambda doubled), `rho < 0` fails, so
# the trial loop ends after one trial, and `rho == 0` terminates the round: one iteration, one trial, one rejection in either round.
EXACT_COUNTS = dict(iterations=[1, 1], trials=[1, 1], rejected=[1, 1])


def _exact_keyframes():
    kfs = np.zeros(len(EXACT_LOCAL) + len(EXACT_FIXED), bc.KF_DTYPE)
    for k, (name, t) in enumerate(EXACT_LOCAL + EXACT_FIXED):
        T = bc.pose(EXACT_PRIORS[name], np.array(t)) + 0.0           # + 0.0: no negative zero among the bytes that must come back
        kfs[k]["Tcw"] = T.astype(F32).reshape(16)
        assert np.array_equal(kfs[k]["Tcw"].astype(np.float64), T.reshape(16))
        for key in ("fx", "fy", "cx", "cy", "mbf"):
            kfs[k][key] = EXACT_CAM[key]
    return kfs


def exact_edge(kfs, k, p, X, stereo, du=0.0, weight=1.0, behind=False):
    """The edge of keyframe k on point p at X, observed at its exact projection (+ du in u), or None when k does not see X at depth
    4 / 8 / 16 (behind = True: at a negative depth) inside the image.  Asserts that the observation is exact in f32."""
    T = kfs[k]["Tcw"].reshape(4, 4).astype(np.float64)
    x, y, z = T[:3, :3] @ X + T[:3, 3]
    if (z not in (-4.0, -8.0) if behind else z not in (4.0, 8.0, 16.0)):
        return None
    u, v = 512.0 * x / z + 320.0, 512.0 * y / z + 240.0
    ur = u - 256.0 / z
    if not (0.0 <= u + du <= 640.0 and 0.0 <= v <= 480.0 and ur >= 0.0 and u - abs(du) >= 0.0):
        return None
    e = np.zeros((), bc.EDGE_DTYPE)
    e["kf"], e["point"], e["u"], e["v"], e["ur"], e["inv_sigma2"] = k, p, u + du, v, ur if stereo else -1.0, weight
    assert float(e["u"]) == u + du and float(e["v"]) == v and (not stereo or (float(e["ur"]) == ur and ur >= 0.0))
    return e


def exact_scene(kind, n_points=40, seed=5):
    """The exact scene: kind = mono / stereo / mixed.  Edges point by point, keyframes ascending; the start is the truth."""
    rng = np.random.default_rng(seed)
    kfs = _exact_keyframes()
    X = np.stack([rng.integers(-16, 17, n_points) / 16.0, rng.integers(-16, 17, n_points) / 16.0, rng.choice([4.0, 8.0, 16.0], n_points)], 1)
    edges = []
    for p in range(n_points):
        for k in range(len(kfs)):
            stereo = kind == "stereo" or (kind == "mixed" and (p + k) % 2 == 0)
            e = exact_edge(kfs, k, p, X[p], stereo)
            if e is not None:
                edges.append(e)
    edges = np.array(edges, bc.EDGE_DTYPE)
    edges["tag"] = np.arange(len(edges))
    xw = X.astype(F32)
    assert np.array_equal(xw.astype(np.float64), X)
    per_kf, per_pt = np.bincount(edges["kf"], minlength=len(kfs)), np.bincount(edges["point"], minlength=n_points)
    # every orientation, local and fixed, is in use, and every local pose is well determined
    assert per_kf[:len(EXACT_LOCAL)].min() >= 12 and per_kf.min() >= 6 and per_pt.min() >= 3, (per_kf, per_pt)
    ref = np.where(np.arange(n_points) % 7 == 0, -1, np.arange(n_points) % len(kfs)).astype(np.int32)
    return dict(kfs=kfs, n_local=len(EXACT_LOCAL), xw=xw, edges=edges, ref_kf=ref, gt_xw=X)


def _case(scene, level1=None, erase=None, chi2=(0.0, 0.0)):
    n = len(scene["edges"])
    level1 = np.zeros(n, np.uint8) if level1 is None else np.asarray(level1, np.uint8)
    return dict(scene=scene, level1=level1, erase=level1.copy() if erase is None else np.asarray(erase, np.uint8), counts=EXACT_COUNTS, chi2=chi2)


def probe_thresholds():
    """The exact mixed scene plus pairs of duplicate edges (DESIGN Q32 allows them): same keyframe, point and weight w, observed at
    u = proj + 1 and u = proj - 1.  Their gradients cancel exactly in every summation order, so nothing moves, and each edge's chi2 is
    1 * (w * 1) = w exactly.  The flags are written down from the DOUBLE compare chi2 > 5.991 | 7.815: float(5.991) = 5.99100017... is
    above 5.991 (an outlier here, an inlier under PoseOptimization's f32 compare), the f32 one step below is not; likewise 7.815."""
    s = exact_scene("mixed", seed=6)
    kfs, X = s["kfs"], s["gt_xw"]
    below = lambda x: np.nextafter(F32(x), F32(0))
    rows = [(False, F32(CHI2_MONO), 1), (False, below(CHI2_MONO), 0), (True, F32(CHI2_STEREO), 1), (True, below(CHI2_STEREO), 0), (True, F32(7.0), 0)]
    assert float(F32(CHI2_MONO)) > CHI2_MONO > float(below(CHI2_MONO)) and float(F32(CHI2_STEREO)) > CHI2_STEREO > float(below(CHI2_STEREO))
    extra, flags, chi2_round2 = [], [], 0.0
    p = 0
    for k in (1, 6, 3, 4):                                   # a local and a fixed half turn, a local half_z, the fixed identity
        for stereo, w, flag in rows:
            while True:                                      # the next point this keyframe sees with room for u +- 1
                pair = [exact_edge(kfs, k, p, X[p], stereo, du=du, weight=w) for du in (1.0, -1.0)]
                p = (p + 1) % len(X)
                if pair[0] is not None and pair[1] is not None:
                    break
            extra += pair; flags += [flag, flag]
            chi2_round2 += 0.0 if flag else 2.0 * float(w)  # f32 values of one magnitude: their f64 sum is exact in any order
    extra = np.array(extra, bc.EDGE_DTYPE)
    extra["tag"] = 5000 + np.arange(len(extra))
    n0 = len(s["edges"])
    at = n0 // 2                                             # the pairs go into the middle of the edge list
    s["edges"] = np.concatenate([s["edges"][:at], extra, s["edges"][at:]])
    level1 = np.zeros(len(s["edges"]), np.uint8)
    level1[at:at + len(extra)] = flags
    assert level1.sum() == 16
    return _case(s, level1, chi2=(None, chi2_round2))


def probe_depth():
    """Points BEHIND a keyframe (depth -4) observed at their exact projection: chi2 = 0, uR >= 0, no force, nothing moves -- the edge
    is flagged by !isDepthPositive() alone.  A local keyframe (0, identity; 3, half_z) and a fixed one (7, half_z), mono and stereo;
    the half turns 1 and 2 (local) and the fixed identity 4 see the same points in front of them."""
    s = exact_scene("mixed", seed=7)
    kfs, n = s["kfs"], len(s["xw"])
    Xb = np.array([[0.25, -0.5, -4.0], [-0.75, 0.125, -4.0], [0.5, 0.5, -4.0]])
    extra, flags = [], []
    for j, X in enumerate(Xb):
        for k in (1, 2, 4):
            e = exact_edge(kfs, k, n + j, X, stereo=(j + k) % 2 == 0)
            assert e is not None
            extra.append(e); flags.append(0)
        for k, stereo in ((0, j == 0), (3, j == 1), (7, j != 1)):
            e = exact_edge(kfs, k, n + j, X, stereo=stereo, behind=True)
            assert e is not None
            extra.append(e); flags.append(1)
    extra = np.array(extra, bc.EDGE_DTYPE)
    extra["tag"] = 6000 + np.arange(len(extra))
    s["xw"] = np.concatenate([s["xw"], Xb.astype(F32)]); s["gt_xw"] = np.concatenate([s["gt_xw"], Xb])
    s["ref_kf"] = np.concatenate([s["ref_kf"], np.array([0, -1, 7], np.int32)])
    level1 = np.concatenate([np.zeros(len(s["edges"]), np.uint8), np.array(flags, np.uint8)])
    s["edges"] = np.concatenate([s["edges"], extra])
    assert level1.sum() == 9
    return _case(s, level1)


def last_trial_rejected():
    """Round 1 ends on a REJECTED trial whose cached errors differ from the fresh ones -- built, not searched, because no seed can give
    it: with finite numbers a round's last trial is rejected only after ten rejections in a row (or rho == 0), by when lambda has grown
    2^45-fold and the rejected step is nil, so cached and fresh chi2 agree to ~1e-10 (and rho is rounding noise, inside the margin).
    What is left is the non-finite path (the BA counterpart of pose_crafted's depth_zero, DESIGN Q24b): a point ON the plane of local
    keyframe 0 makes its mono error infinite, every sum NaN and every trial of round 1 rejected (rho = NaN is neither > 0 nor < 0 nor
    == 0: five iterations of one rejected trial each).  The estimates are restored, but every cached chi2 is the NaN of the rejected
    trial, and NaN > bound is false: a pair of duplicate edges at u = proj +- 8 (chi2 = 64 each, cancelling gradients) is NOT sent to
    level 1.  The on-plane edge is, by its depth; round 2 is then finite and at its optimum, ends by rho == 0 and erases the pair."""
    s = exact_scene("mixed", seed=8)
    kfs, n = s["kfs"], len(s["xw"])
    Xp = np.array([0.5, 0.25, 0.0])
    on_plane = np.zeros((), bc.EDGE_DTYPE)
    on_plane["kf"], on_plane["point"], on_plane["u"], on_plane["v"], on_plane["ur"], on_plane["inv_sigma2"] = 0, n, 320.0, 240.0, -1.0, 1.0
    seen = exact_edge(kfs, 4, n, Xp, stereo=True)
    pairs = [[exact_edge(kfs, 2, p, s["gt_xw"][p], stereo=False, du=du) for du in (8.0, -8.0)] for p in range(n)]
    pair = [q for q in pairs if q[0] is not None and q[1] is not None][0]             # the first point local keyframe 2 sees
    assert seen is not None
    extra = np.array([on_plane, seen] + pair, bc.EDGE_DTYPE)
    extra["tag"] = 7000 + np.arange(4)
    n0 = len(s["edges"])
    s["edges"] = np.concatenate([s["edges"], extra])
    s["xw"] = np.concatenate([s["xw"], Xp.astype(F32)[None]]); s["gt_xw"] = np.concatenate([s["gt_xw"], Xp[None]])
    s["ref_kf"] = np.concatenate([s["ref_kf"], np.array([4], np.int32)])
    level1 = np.zeros(n0 + 4, np.uint8); level1[n0] = 1
    erase = level1.copy(); erase[n0 + 2:] = 1
    c = _case(s, level1, erase, chi2=(float("inf"), 128.0))           # round 1 keeps the chi2 of the restored estimates: infinite
    c["counts"] = dict(iterations=[5, 1], trials=[5, 1], rejected=[5, 1])
    c["pair"] = np.array([n0 + 2, n0 + 3])
    return c


EXACT = {"exact_mono": lambda: _case(exact_scene("mono")), "exact_stereo": lambda: _case(exact_scene("stereo")),
         "exact_mixed": lambda: _case(exact_scene("mixed")), "probe_thresholds": probe_thresholds, "probe_depth": probe_depth,
         "last_trial_rejected": last_trial_rejected}
# Every one of them is exempt from the margin rule, as pose_crafted's on_threshold cases are: it sits on a threshold on purpose (rho == 0
# in all of them, chi2 on its bound in probe_thresholds, a depth of 0 in last_trial_rejected) and nothing moves.
ON_THRESHOLD = tuple(EXACT)


# ---------------------------------------------------------------- cached-error cases: seeded, searched
def fresh_chi2(prob, Tcw, xw):
    """Every edge's chi2 at the returned estimates -- the local keyframes' f32 Tcw (n_local, 4, 4), the fixed cameras' table entries, the
    f32 points -- in plain numpy f64: the textbook reprojection error, no code shared with the oracle."""
    e, kfs = prob["edges"], prob["kfs"]
    T = np.array(kfs["Tcw"]).reshape(-1, 4, 4).astype(np.float64)
    T[:prob["n_local"]] = np.asarray(Tcw, np.float64)
    Tk = T[e["kf"]]
    pc = np.einsum("eij,ej->ei", Tk[:, :3, :3], np.asarray(xw, np.float64)[e["point"]]) + Tk[:, :3, 3]
    cam = {k: kfs[k][e["kf"]].astype(np.float64) for k in ("fx", "fy", "cx", "cy", "mbf")}
    with np.errstate(divide="ignore", invalid="ignore"):           # a point on a camera plane (last_trial_rejected) has no finite error
        pu = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]
        pv = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        r2 = (e["u"] - pu) ** 2 + (e["v"] - pv) ** 2
        stereo = e["ur"] >= 0
        r2 = r2 + np.where(stereo, (e["ur"] - (pu - cam["mbf"] / pc[:, 2])) ** 2, 0.0)
        return e["inv_sigma2"].astype(np.float64) * r2


def bounds_of(prob):
    return np.where(prob["edges"]["ur"] < 0, CHI2_MONO, CHI2_STEREO)


def point_stays_active(prob, level1):
    """Per edge: its point keeps a level-0 edge for round 2."""
    left = np.bincount(prob["edges"]["point"][level1 == 0], minlength=len(prob["xw"]))
    return left[prob["edges"]["point"]] > 0


def stale_level1_edges(prob, result):
    """The edges that show the cached-error rule for level-1 edges (Q33): sent to level 1 after round 1 while their point stays active
    in round 2, erased all the same -- although their chi2 at the returned estimates is below half their bound."""
    fresh = fresh_chi2(prob, result["Tcw"], result["xw"])
    return np.flatnonzero((result["level1"] == 1) & point_stays_active(prob, result["level1"]) & (result["erase"] == 1)
                          & (fresh < 0.5 * bounds_of(prob)))


def well_posed(scene, result=None):
    """The conditions of every seeded case (not measurements): every decision at least MARGIN from its threshold, no oracle variant takes
    another decision, a spread below the sanity cap of test_tolerance_yardstick_is_recorded.  -> the spread, or None."""
    prob = bc.problem_of(scene)
    r = result or bc.run_oracle(prob)
    if min(r["margins"].values()) < bc.MARGIN or r["branches"]["factor_fail"]:
        return None
    sp = bc.spread_of(prob, r)
    return sp if sp is not None and max(sp.values()) < 2e-5 else None


def pick(build, want, seeds):
    """The first seed whose scene the oracle takes where `want(scene, result)` says and which is well_posed(); in the style of
    pnp_cases.pick.  A seed that fails a condition is replaced by the next, never skipped by a test."""
    for seed in seeds:
        s = build(seed)
        r = bc.run_oracle(bc.problem_of(s))
        if want(s, r) and well_posed(s, r) is not None:
            s["seed"] = seed
            return s
    raise AssertionError("no seed gives a well-posed scene on the wanted branch")


def build_stale(seed):
    # a start far enough off that round 1's five iterations end short of the optimum: good edges still above their bound go to level 1
    return bc.make_scene(seed, 3, 2, 30, stereo_frac=0.5, pose_noise=(0.2, 0.8), point_noise=1.0, mild=0.0)


def want_stale(s, r):
    return r["branches"]["level1_point_active"] > 0 and len(stale_level1_edges(bc.problem_of(s), r)) > 0


def build_rejected(seed):
    return bc.make_scene(seed, 3, 2, 30, stereo_frac=0.5, noise=1.0, pose_noise=(0.1, 0.5), point_noise=0.8, mild=0.05)


def build_between(seed):
    return bc.make_scene(seed, 3, 2, 30, stereo_frac=0.8, noise=1.0, mild=0.0)


# (build, want, the seeds the search walks).  The first seed that passes is the case; the search is deterministic.
SEARCHED = {"stale_level1": (build_stale, want_stale, range(500, 560)),
            "stereo_between": (build_between, lambda s, r: r["branches"]["stereo_between"] > 0, range(600, 660))}


# ---------------------------------------------------------------- orders, list lengths and sizes
ORDERS = ("point_major", "kf_major", "shuffled", "reversed")


def reordered(scene, order, seed=0):
    """The same scene with its edges in another insertion order (`planted` follows)."""
    e = scene["edges"]
    perm = {"point_major": lambda: np.arange(len(e)), "kf_major": lambda: np.argsort(e["kf"], kind="stable"),
            "shuffled": lambda: np.random.default_rng(seed).permutation(len(e)), "reversed": lambda: np.arange(len(e))[::-1]}[order]()
    s = dict(scene)
    s["edges"] = np.ascontiguousarray(e[perm])
    inv = np.empty(len(e), np.int64); inv[perm] = np.arange(len(e))
    s["planted"] = np.sort(inv[scene["planted"]])
    return s


def thinned(seed, n_local, n_fixed, n_points, keep, **kw):
    """make_scene with every keyframe seeing every point, thinned to the edges keep(kf, point, rng) -> bool array selects."""
    s = bc.make_scene(seed, n_local, n_fixed, n_points, **kw)
    e = s["edges"]
    mask = np.asarray(keep(e["kf"], e["point"], np.random.default_rng(seed + 7)), bool)
    was = np.zeros(len(e), bool); was[s["planted"]] = True
    s = bc.drop_edges(s, mask)
    s["planted"] = np.flatnonzero(was[mask])
    return s


def scene_orders(order):
    """3 local + 2 fixed keyframes, 60 points, 300 edges, in one of the four insertion orders."""
    return reordered(bc.make_scene(701, 3, 2, 60, stereo_frac=0.5), order, seed=701)


def scene_same_key_chunk(n):
    """Keyframe-major with n edges on every keyframe: n = 256 fills each 256-edge chunk of the stable fill with ONE key, n = 257 moves
    every chunk boundary into a keyframe's list, one edge further each time."""
    return reordered(bc.make_scene(710 + n, 3, 2, n, stereo_frac=0.6), "kf_major")


LIST_LENGTHS = (63, 64, 65, 129)


def scene_list_lengths():
    """Local keyframe k sees the first LIST_LENGTHS[k] points (a wave-strided pose gather of 63 / 64 / 65 / 129 edges), the two fixed
    cameras see all 129; keyframe-major, so every list is also split by a chunk boundary somewhere else."""
    L = np.array(LIST_LENGTHS + (129, 129))
    return reordered(thinned(720, 4, 2, 129, lambda kf, pt, rng: pt < L[kf], stereo_frac=0.6), "kf_major")


def scene_size(n_local, n_fixed, n_points, obs, seed):
    """n_local local keyframes (6 n_local rows of the reduced system), every point seen by `obs` keyframes -- and point 0 by all of
    them: at the caps that is one key on 192 edges."""
    def keep(kf, pt, rng):
        K = n_local + n_fixed
        sees = np.zeros((n_points, K), bool)
        for p in range(n_points):
            sees[p, rng.choice(K, obs, replace=False)] = True
        sees[0] = True
        return sees[pt, kf]
    return thinned(seed, n_local, n_fixed, n_points, keep, stereo_frac=0.6)


def scene_block_sparse():
    """Two groups of local keyframes that share no point (0-2 on points 0-29, 3-5 on points 30-47: S is block diagonal but for
    nothing), and local keyframe 6 on points 48-59, which no other local keyframe sees; the two fixed cameras see every point."""
    def keep(kf, pt, rng):
        group = np.where(pt < 30, 0, np.where(pt < 48, 1, 2))
        return (kf >= 7) | ((kf < 3) & (group == 0)) | ((kf >= 3) & (kf < 6) & (group == 1)) | ((kf == 6) & (group == 2))
    return thinned(730, 7, 2, 60, keep, stereo_frac=0.6)


def scene_fixed_byte(byte):
    """The same problem with the `fixed` byte of the fixed cameras 0 or 1: fixed whatever the byte says (Q32)."""
    s = bc.make_scene(740, 3, 3, 40, stereo_frac=0.5)
    s["kfs"] = s["kfs"].copy()
    s["kfs"]["fixed"][s["n_local"]:] = byte
    return s


MAX_LOCAL, MAX_FIXED = 64, 128                               # SD_BA_MAX_LOCAL, SD_BA_MAX_FIXED of k_ba.h
SCENES = {
    **{"order_" + o: (lambda o=o: scene_orders(o)) for o in ORDERS},
    "chunk_256": lambda: scene_same_key_chunk(256),
    "chunk_257": lambda: scene_same_key_chunk(257),
    "list_lengths": scene_list_lengths,
    "size_16": lambda: scene_size(16, 3, 80, 6, 750),
    "size_63": lambda: scene_size(63, 3, 260, 8, 751),
    "size_caps": lambda: scene_size(MAX_LOCAL, MAX_FIXED, 300, 14, 752),
    "block_sparse": scene_block_sparse,
    "fixed_byte_0": lambda: scene_fixed_byte(0),
    "fixed_byte_1": lambda: scene_fixed_byte(1),
}

_scenes, _results, _exact = {}, {}, {}


def exact_case(name):
    if name not in _exact:
        _exact[name] = EXACT[name]()
    return _exact[name]


def scene(name):
    """A SEARCHED or SCENES scene by name, built (searched) once."""
    if name not in _scenes:
        _scenes[name] = pick(*SEARCHED[name]) if name in SEARCHED else SCENES[name]()
    return _scenes[name]


def expected(name):
    """The oracle's answer for an EXACT, SEARCHED or SCENES case, computed once and shared; not to be modified."""
    if name not in _results:
        s = exact_case(name)["scene"] if name in EXACT else scene(name)
        _results[name] = bc.run_oracle(bc.problem_of(s))
    return _results[name]


def assert_by_construction(name, got):
    """What an EXACT case states, against a result of the oracle's or the device's layout."""
    c = exact_case(name)
    s = c["scene"]
    assert got["Tcw"].astype(F32).tobytes() == s["kfs"]["Tcw"][:s["n_local"]].tobytes(), "%s: a pose moved" % name
    assert got["xw"].tobytes() == s["xw"].tobytes(), "%s: a point moved" % name
    assert np.array_equal(got["level1"], c["level1"]), (name, np.flatnonzero(got["level1"] != c["level1"]))
    assert np.array_equal(got["erase"], c["erase"]), (name, np.flatnonzero(got["erase"] != c["erase"]))
    st = got["stats"]
    assert st["n_level1"] == c["level1"].sum() and st["n_erased"] == c["erase"].sum()
    for f, want in c["counts"].items():
        assert st[f].tolist() == want, (name, f, st[f])
    for rnd, want in enumerate(c["chi2"]):
        assert want is None or st["chi2"][rnd] == want, (name, rnd, st["chi2"][rnd])
