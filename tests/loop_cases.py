"""Shared by test_loop_oracle.py, test_gpu_loop.py, tools/fuzz_loop.py and tools/bench_loop.py: the CPU oracle of the loop-closing
matchers (tests/cpp/loop_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory), numpy restatements of the
three functions, and seeded crafted scenes.

Scw scenes are the scenes of fuse_cases.py (keyframes, points, jobs (keyframe, entries, state)) plus, per job, a similarity
scw[j] = [s * Rcw | s * tcw] of the keyframe's pose and an incoming vpMatched row matched[j] (None = all NULL): the same scene runs
through Fuse(pKF, Scw, ...) and SearchByProjection(pKF, Scw, ...).  BoW cases are pairs of keyframes built from the identities and
candidates of triangulate_cases.Descriptors, so that node membership and every distance that matters are chosen.
Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import fuse_cases as fc
import triangulate_cases as tc
from fuse_cases import ADD, MEET_BAD, MEET_CANDIDATE, MEET_KF, HIT_DTYPE, MP_DTYPE, SceneBuilder, flipped, rand_desc
from triangulate_cases import CAM, F32, KP_DTYPE, KeyFrameBuilder, Levels, T1_DEFAULT, _p

ROOT = tc.ROOT
BRANCHES = ["entry_skip", "searched", "z_negative", "z_zero", "out_of_image", "u_eq_maxx", "u_eq_minx", "v_eq_maxy", "v_eq_miny", "dist_below_min",
            "dist_above_max", "view_angle", "window_empty", "clip_left", "clip_right", "clip_top", "clip_bottom", "octave_below", "octave_above",
            "octave_lm1", "octave_l", "tie_earlier_wins", "dist50", "dist51", "no_features", "empty_job", "window_over_64", "window_over_16_cols",
            "fuse_dist256", "meet_kf", "meet_bad", "add", "meet_candidate", "chi2_would_reject",
            "already_found", "target_matched", "taken_by_earlier", "loser_second_choice", "loser_above_th", "loser_nothing_left",
            "bow_node_shared", "bow_only_in_1", "bow_only_in_2", "bow_invalid1", "bow_invalid2", "bow_taken2", "bow_dist49", "bow_dist50",
            "bow_ratio_pass", "bow_ratio_fail", "bow_single", "bow_tie", "bow_bin_wrap", "bow_culled", "bow_empty_fv", "bow_node2_over_64",
            "bow_node2_over_128", "bow_node1_over_64", "bow_maxima_tie"]
TWINS = dict(none=0, bow_le_th_low=1, bow_index_by_side2=2, fuse_keeps_chi2=3, later_candidate_wins=4, tie_to_later_visit=5)
TH_LOW, HISTO = 50, 30
SCALES = (1.0, 0.5, 2.0, 1.37)

_oracles = {}


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast (to count the decisions that changes)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="loop_oracle_")
        so = os.path.join(d, "libloop_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []          # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "loop_oracle.cpp")])
        L = C.CDLL(so)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.sd_loop_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_loop_oracle_set_twin.argtypes = [i]
        L.sd_loop_oracle_decompose.argtypes = [vp, vp]
        L.sd_loop_oracle_kf_new.restype = vp
        L.sd_loop_oracle_kf_new.argtypes = [i, vp, vp, vp, vp, i, vp, vp, i, vp, vp]
        L.sd_loop_oracle_kf_free.argtypes = [vp]
        L.sd_loop_oracle_fuse.argtypes = [vp, vp, i, vp, vp, vp, vp, f, vp, vp, vp]
        L.sd_loop_oracle_project.argtypes = [vp, vp, i, vp, vp, vp, vp, i, vp, vp]
        L.sd_loop_oracle_bow.argtypes = [vp, vp, vp, vp, f, i, vp]
        assert L.sd_loop_oracle_branch_count() == len(BRANCHES)
        _oracles[contract] = L
    return _oracles[contract]


def branches(L):
    b = L.sd_loop_oracle_branches()
    return {name: int(b[i]) for i, name in enumerate(BRANCHES)}


class OracleKF:
    def __init__(self, L, kf, cam=CAM, lv=None):
        lv = lv or Levels()
        self.L, self.N = L, len(kf["kp"])
        kp = np.ascontiguousarray(kf["kp"], KP_DTYPE); d = np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1); ur = np.ascontiguousarray(kf["ur"], F32)
        c = fc.cam_array(cam); iv = fc.inv_sigma2(lv)
        fv = kf.get("fv")
        fn = np.ascontiguousarray(fv[0], np.uint32) if fv is not None else np.zeros(0, np.uint32)
        ff = np.ascontiguousarray(fv[1], np.uint32) if fv is not None else np.zeros(0, np.uint32)
        self.h = L.sd_loop_oracle_kf_new(self.N, _p(kp), _p(d), _p(ur), _p(c), lv.nlevels, _p(lv.scale), _p(iv), len(fn), _p(fn), _p(ff))

    def close(self):
        self.L.sd_loop_oracle_kf_free(self.h)


def decompose(Scw, contract="off"):
    T = np.zeros(16, F32)
    oracle(contract).sd_loop_oracle_decompose(_p(np.ascontiguousarray(Scw, F32).reshape(16)), _p(T))
    return T.reshape(4, 4)


def decompose_numpy(Scw):
    """DESIGN.md Q41 restated."""
    S = np.asarray(Scw, F32).reshape(4, 4)
    scw = F32(np.sqrt(np.float64(S[0, 0]) * np.float64(S[0, 0]) + np.float64(S[0, 1]) * np.float64(S[0, 1]) + np.float64(S[0, 2]) * np.float64(S[0, 2])))
    inv = F32(1.0 / np.float64(scw))
    T = np.eye(4, dtype=F32)
    T[:3] = (S[:3] * inv).astype(F32)
    return T


# ---------------------------------------------------------------- Scw scenes
def similarity(T, s):
    """Scw = [s Rcw | s tcw] in f32, formed in f64."""
    S = np.asarray(T, np.float64).copy()
    S[:3] *= float(s)
    return S.astype(F32)


def with_scale(scene, s, matched=None):
    sc = dict(scene)
    sc["scw"] = [similarity(scene["kfs"][j[0]]["Tcw"], s) for j in scene["jobs"]]
    sc["matched"] = matched if matched is not None else [None] * len(scene["jobs"])
    sc["name"] = "%s_s%g" % (scene["name"], s)
    return sc


def matched_from_state(scene, extra=None):
    """An incoming vpMatched row per job from the job's feature states: a feature that holds a point holds one outside the table (-2);
    extra = {(job, feature): point index}."""
    rows = []
    for q, (k, entries, state) in enumerate(scene["jobs"]):
        n = len(scene["kfs"][k]["kp"])
        m = np.full(n, -1, np.int32)
        if state is not None:
            m[np.asarray(state[:n]) != 0] = -2
        for (job, f), p in (extra or {}).items():
            if job == q:
                m[f] = p
        rows.append(m)
    return rows


def cpu_fuse(scene, contract="off", twin="none", cam=CAM, lv=None):
    """Every job through the sequential Fuse(pKF, Scw, ...) -> ([(best, hits, nfused)], branches)."""
    L = oracle(contract)
    okfs = [OracleKF(L, k, cam, lv) for k in scene["kfs"]]
    L.sd_loop_oracle_reset_branches(); L.sd_loop_oracle_set_twin(TWINS[twin])
    p = np.ascontiguousarray(scene["points"], MP_DTYPE); d = np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1)
    out = []
    for q, (k, entries, state) in enumerate(scene["jobs"]):
        n = len(entries)
        e = np.ascontiguousarray(entries, np.int32); S = np.ascontiguousarray(scene["scw"][q], F32).reshape(16)
        best = np.zeros((max(n, 1), 2), np.int32); hits = np.zeros(max(n, 1), HIT_DTYPE); nh = np.zeros(1, np.int32)
        st = np.ascontiguousarray(state, np.uint8) if state is not None else None
        nf = L.sd_loop_oracle_fuse(okfs[k].h, _p(S), n, _p(e), _p(p), _p(d), _p(st), scene.get("th", 3.0), _p(best), _p(hits), _p(nh))
        assert nf == nh[0]
        out.append((best[:n].copy(), hits[:nh[0]].copy(), nf))
    br = branches(L)
    L.sd_loop_oracle_set_twin(0)
    for o in okfs:
        o.close()
    return out, br


def cpu_project(scene, contract="off", twin="none", cam=CAM, lv=None, cap=None):
    """Every job through the sequential SearchByProjection(pKF, Scw, ...) -> ([(assigned (cap or N,), best, nmatches)], branches)."""
    L = oracle(contract)
    okfs = [OracleKF(L, k, cam, lv) for k in scene["kfs"]]
    L.sd_loop_oracle_reset_branches(); L.sd_loop_oracle_set_twin(TWINS[twin])
    p = np.ascontiguousarray(scene["points"], MP_DTYPE); d = np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1)
    out = []
    for q, (k, entries, _) in enumerate(scene["jobs"]):
        n, N = len(entries), okfs[k].N
        e = np.ascontiguousarray(entries, np.int32); S = np.ascontiguousarray(scene["scw"][q], F32).reshape(16)
        m = scene["matched"][q]
        m = np.full(max(N, 1), -1, np.int32) if m is None else np.ascontiguousarray(m, np.int32)
        assigned = np.full(max(cap or N, 1), -1, np.int32); best = np.zeros((max(n, 1), 2), np.int32)
        nm = L.sd_loop_oracle_project(okfs[k].h, _p(S), n, _p(e), _p(p), _p(d), _p(m), int(scene.get("th_proj", 10)), _p(assigned), _p(best))
        out.append((assigned[:cap or N].copy(), best[:n].copy(), nm))
    br = branches(L)
    L.sd_loop_oracle_set_twin(0)
    for o in okfs:
        o.close()
    return out, br


# ---------------------------------------------------------------- numpy restatements (Scw functions)
def _hamming_rows(d, D):
    return np.unpackbits(np.bitwise_xor(D, d[None, :]), axis=1).sum(1).astype(np.int64) if len(D) else np.zeros(0, np.int64)


class NumpyKF:
    """The grid and GetFeaturesInArea of one keyframe in numpy (f32 steps as in DESIGN.md Q31)."""

    def __init__(self, kf, cam=CAM, lv=None):
        self.kf, self.cam, self.lv = kf, cam, lv or Levels()
        k = kf["kp"]
        self.wi = F32(fc.GRID_COLS) / F32(cam["mnMaxX"] - cam["mnMinX"]); self.hi = F32(fc.GRID_ROWS) / F32(cam["mnMaxY"] - cam["mnMinY"])
        nx = (k["x"] - cam["mnMinX"]) * self.wi
        px = np.where(nx < 0, -np.floor(-nx.astype(F32) + F32(0.5)), np.floor(nx.astype(F32) + F32(0.5))).astype(np.int64)
        ny = (k["y"] - cam["mnMinY"]) * self.hi
        py = np.where(ny < 0, -np.floor(-ny.astype(F32) + F32(0.5)), np.floor(ny.astype(F32) + F32(0.5))).astype(np.int64)
        ok = (px >= 0) & (px < fc.GRID_COLS) & (py >= 0) & (py < fc.GRID_ROWS)
        idx = np.nonzero(ok)[0]
        order = np.lexsort((idx, py[idx], px[idx]))              # cell column-major, then insertion order
        self.order, self.px, self.py = idx[order], px, py

    def area(self, u, v, r):
        cam = self.cam
        x0 = max(0, int(np.floor((F32(F32(u - cam["mnMinX"]) - r)) * self.wi))); x1 = min(fc.GRID_COLS - 1, int(np.ceil(F32(F32(u - cam["mnMinX"]) + r) * self.wi)))
        y0 = max(0, int(np.floor((F32(F32(v - cam["mnMinY"]) - r)) * self.hi))); y1 = min(fc.GRID_ROWS - 1, int(np.ceil(F32(F32(v - cam["mnMinY"]) + r) * self.hi)))
        if x0 >= fc.GRID_COLS or x1 < 0 or y0 >= fc.GRID_ROWS or y1 < 0:
            return np.zeros(0, np.int64)
        o = self.order
        sel = o[(self.px[o] >= x0) & (self.px[o] <= x1) & (self.py[o] >= y0) & (self.py[o] <= y1)]
        k = self.kf["kp"][sel]
        return sel[(np.abs(k["x"] - u) < r) & (np.abs(k["y"] - v) < r)]


def _window_numpy(K, T, mp, th):
    """-> (indices in visiting order that pass the level gate) or None for a `continue`."""
    cam, lv = K.cam, K.lv
    X = mp["xw"].astype(F32)
    pc = [F32(F32(F32(T[i, 0] * X[0]) + F32(T[i, 1] * X[1])) + F32(T[i, 2] * X[2])) + T[i, 3] for i in range(3)]
    if pc[2] < 0:
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F32(1) / pc[2]
        u = F32(cam["fx"] * F32(pc[0] * invz)) + cam["cx"]; v = F32(cam["fy"] * F32(pc[1] * invz)) + cam["cy"]
    if not (u >= cam["mnMinX"] and u < cam["mnMaxX"] and v >= cam["mnMinY"] and v < cam["mnMaxY"]):
        return None
    Ow = [F32(F32(F32(-T[0, i]) * T[0, 3]) + F32(F32(-T[1, i]) * T[1, 3])) + F32(F32(-T[2, i]) * T[2, 3]) for i in range(3)]
    PO = np.array([X[i] - Ow[i] for i in range(3)], F32).astype(np.float64)
    dist = F32(np.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]))
    if dist < F32(0.8) * mp["min_distance"] or dist > F32(1.2) * mp["max_distance"]:
        return None
    nrm = mp["normal"].astype(np.float64)
    if PO[0] * nrm[0] + PO[1] * nrm[1] + PO[2] * nrm[2] < 0.5 * np.float64(dist):
        return None
    ratio = F32(mp["max_distance"]) / dist
    level = int(np.ceil(F32(F32(np.log(np.float64(ratio))) / F32(np.log(np.float64(lv.scale[1]))))))
    level = min(max(level, 0), lv.nlevels - 1)
    r = F32(th) * lv.scale[level]
    sel = K.area(u, v, r)
    octv = K.kf["kp"]["octave"][sel]
    return sel[(octv >= level - 1) & (octv <= level)], len(sel)


def numpy_fuse(scene, cam=CAM, lv=None):
    out = []
    for q, (k, entries, state) in enumerate(scene["jobs"]):
        K = NumpyKF(scene["kfs"][k], cam, lv); T = decompose_numpy(scene["scw"][q])
        N = len(K.kf["kp"])
        holds = np.full(N, -1, np.int64)
        if state is not None:
            holds[np.asarray(state[:N]) == 1] = -2; holds[np.asarray(state[:N]) == 2] = -3
        best = np.tile(np.array([-1, 256], np.int32), (len(entries), 1)); hits = []
        for i, m in enumerate(entries):
            if m < 0:
                continue
            w = _window_numpy(K, T, scene["points"][m], scene.get("th", 3.0))
            if w is None or not len(w[0]):
                continue
            d = _hamming_rows(scene["pdesc"][m], K.kf["desc"][w[0]])
            j = int(np.argmin(d))                                # the first minimum in visiting order
            best[i] = (w[0][j], d[j])
            if d[j] <= TH_LOW:
                f = int(w[0][j])
                if holds[f] == -1:
                    hits.append((i, f, d[j], ADD, -1)); holds[f] = i
                else:
                    hits.append((i, f, d[j], {-2: MEET_KF, -3: MEET_BAD}.get(int(holds[f]), MEET_CANDIDATE), holds[f] if holds[f] >= 0 else -1))
        out.append((best, np.array(hits, HIT_DTYPE) if hits else np.zeros(0, HIT_DTYPE), len(hits)))
    return out


def numpy_project(scene, cam=CAM, lv=None):
    out = []
    for q, (k, entries, _) in enumerate(scene["jobs"]):
        K = NumpyKF(scene["kfs"][k], cam, lv); T = decompose_numpy(scene["scw"][q])
        N = len(K.kf["kp"])
        m0 = scene["matched"][q]
        vp = np.full(N, -1, np.int64) if m0 is None else np.asarray(m0[:N], np.int64).copy()
        found = set(int(x) for x in vp if x >= 0)
        assigned = np.full(N, -1, np.int32)
        best = np.tile(np.array([-1, 256], np.int32), (len(entries), 1)); nm = 0
        for i, m in enumerate(entries):
            if m < 0 or int(m) in found:
                continue
            w = _window_numpy(K, T, scene["points"][m], scene.get("th_proj", 10))
            if w is None:
                continue
            sel = w[0][vp[w[0]] == -1]
            if not len(sel):
                continue
            d = _hamming_rows(scene["pdesc"][m], K.kf["desc"][sel])
            j = int(np.argmin(d))
            if d[j] < 256:
                best[i] = (sel[j], d[j])
                if d[j] <= TH_LOW:
                    vp[sel[j]] = m; assigned[sel[j]] = i; nm += 1
        out.append((assigned, best, nm))
    return out


# ---------------------------------------------------------------- crafted Scw scenes
def crafted_scene():
    """The crafted scene of fuse_cases.py (every branch of the shared search, the four actions) plus what the Scw functions add:
    a lone member at distance 256, the level gate from level - 2 to level + 1, a window clipped on the left, windows of 64 / 65 members,
    v on mnMaxY (windows of 16 / 17 columns: wide_window_scene).  Job 0 keyframe A, job 1 keyframe I (identity pose, depth 1), job 2 a
    keyframe without features, job 3 empty, job 4 keyframe A again with the added cases, job 5 keyframe I with the v bound."""
    base = fc.crafted_scene()
    sc = dict(base)                                              # the same keyframes and points, more of both
    A, I = 0, 1
    rng = np.random.default_rng(31)
    kfA = _Appender(base["kfs"][A]); kfI = _Appender(base["kfs"][I])
    pts, pdesc = list(base["points"]), list(base["pdesc"])
    ex = {}

    def point(T, u, v, z, level, desc=None, **kw):
        X = tc.from_pixel(np.asarray(T, np.float64), u, v, z)
        pts.append(fc.point_record(np.asarray(T, np.float64), X, level, None, **kw)); pdesc.append(rand_desc(rng) if desc is None else desc)
        return len(pts) - 1

    eA = []
    TA = np.asarray(base["kfs"][A]["Tcw"], np.float64)
    # a lone member at distance 256: the complement of the point's descriptor
    p = point(TA, 200.0, 330.0, 10.0, 2); f = kfA.add(200.0, 330.0, np.bitwise_not(pdesc[p]), 2)
    eA.append(p); ex["dist256"] = (4, len(eA) - 1, f, 256)
    # the level gate: octave level - 2 ... level + 1 for a point predicted at level 3
    for name, octv, hit in (("octave_lm2", 1, False), ("octave_lm1", 2, True), ("octave_l", 3, True), ("octave_lp1", 4, False)):
        u, v = 300.0 + 70.0 * octv, 330.0
        p = point(TA, u, v, 10.0, 3); f = kfA.add(u, v, flipped(pdesc[p], 10, rng), octv)
        eA.append(p); ex[name] = (4, len(eA) - 1, f if hit else -1, 10 if hit else 256)
    # the left border clips the window (the right, bottom and top ones are in the base scene)
    p = point(TA, 3.0, 100.0, 10.0, 2); f = kfA.add(4.0, 100.0, flipped(pdesc[p], 10, rng), 2)
    eA.append(p); ex["clip_left"] = (4, len(eA) - 1, f, 10)
    # windows of 64 and 65 members (one and two passes of the wave), the nearest late in the walk
    for n, u in ((64, 700.0), (65, 800.0)):
        p = point(TA, u, 330.0, 10.0, 2)
        for j in range(n):
            f = kfA.add(u + rng.uniform(-2, 2), 330.0 + rng.uniform(-2, 2), flipped(pdesc[p], 12 if j == n - 3 else int(rng.integers(14, 60)), rng), 2)
            if j == n - 3:
                fb = f
        eA.append(p); ex["window_%d" % n] = (4, len(eA) - 1, fb, 12)
    sc.update(kfs=list(base["kfs"]))
    # keyframe I: v on the image bounds (u is in the base scene)
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    eI = []
    x_mid = float((F32(400.0) - cx) / fx)
    # (no f32 ordinate projects onto mnMinY = 0 exactly with this camera: fl(fy * y) skips -cy.  v_min_scene has a camera that does.)
    for name, target, hit in (("v_eq_maxy", CAM["mnMaxY"], False),):
        y = fc.solve_px(target, fy, cy)
        pts.append(fc.point_record(np.eye(4), [x_mid, float(y), 1.0], 2)); pdesc.append(rand_desc(rng)); p = len(pts) - 1
        f = kfI.add(400.0, float(target) + (1.0 if hit else -1.0), flipped(pdesc[p], 10, rng), 2)
        eI.append(p); ex[name] = (5, len(eI) - 1, f if hit else -1, 10 if hit else 256)
    sc["kfs"][A] = kfA.build(); sc["kfs"][I] = kfI.build()
    sc["points"] = np.array(pts, MP_DTYPE); sc["pdesc"] = np.array(pdesc, np.uint8).reshape(len(pts), 32)
    stA = base["jobs"][0][2]
    st = np.zeros(len(sc["kfs"][A]["kp"]), np.uint8); st[:len(stA)] = stA
    sc["jobs"] = [(base["jobs"][0][0], base["jobs"][0][1], st)] + list(base["jobs"][1:]) + [(A, np.array(eA, np.int32), st), (I, np.array(eI, np.int32), None)]
    sc["expect_scw"] = ex
    sc["name"] = "crafted_scw"
    return sc


# A camera whose principal point an f32 ordinate reaches: cy = fy / 4 (exact), so y = -0.25 at depth 1 gives fl(fy * y) + cy == 0 == mnMinY.
CAM_VMIN = dict(CAM, cy=F32(CAM["fy"] * F32(0.25)))


def v_min_scene():
    """v exactly ON mnMinY (inside: IsInImage has `>=`) and the next f32 ordinate beyond it (outside), under CAM_VMIN and the identity
    pose.  -> scene with expect_scw {name: (job, position, bestIdx, bestDist)}; run it with cam=CAM_VMIN."""
    S = SceneBuilder(4)
    I = S.keyframe(np.eye(4))
    cam = CAM_VMIN
    x_mid = float((F32(400.0) - cam["cx"]) / cam["fx"])
    on = F32(-0.25); beyond = np.nextafter(on, F32(-1))
    assert F32(cam["fy"] * on) + cam["cy"] == cam["mnMinY"] and F32(cam["fy"] * beyond) + cam["cy"] < cam["mnMinY"]
    entries, ex = [], {}
    for name, y, hit in (("v_eq_miny", on, True), ("v_below_miny", beyond, False)):
        S.points.append(fc.point_record(np.eye(4), [x_mid, float(y), 1.0], 2)); S.pdesc.append(rand_desc(S.rng)); p = len(S.points) - 1
        f = S.kfs[I].add(400.0 + (0.0 if hit else 40.0), 1.0, flipped(S.pdesc[p], 10, S.rng), 2)
        entries.append(p); ex[name] = (0, len(entries) - 1, f if hit else -1, 10 if hit else 256)
    S.job(I, entries)
    sc = with_scale(S.build("v_min"), 1.0)
    sc["th_proj"] = 3
    sc["expect_scw"] = ex
    return sc


class _Appender:
    """More features for a built keyframe."""

    def __init__(self, kf):
        self.kf = kf
        self.b = KeyFrameBuilder(kf["Tcw"])
        self.n0 = len(kf["kp"])

    def add(self, *a, **kw):
        return self.n0 + self.b.add(*a, **kw)

    def build(self):
        e = self.b.build()
        out = dict(self.kf)
        for key in ("kp", "desc", "ur", "depth"):
            out[key] = np.concatenate([self.kf[key], e[key]])
        out["has_mp"] = None; out["kp_raw"] = None
        return out


# names of fuse_cases.crafted_scene that the chi-square test of Fuse(pKF, vpMapPoints, th) rejects and the Scw overload accepts
CHI2_ONLY = ("stereo_fails", "mono_fails", "uright_zero")


def check_crafted(scene, fuse_results):
    """The anchors found what they were built to find under Fuse(pKF, Scw, ...) with scale 1."""
    base = fc.crafted_scene()["expect"]
    for name, e in base.items():
        job, pos, idx, dist, action = e[:5]
        got = tuple(int(x) for x in fuse_results[job][0][pos])
        if name in CHI2_ONLY:
            assert got[0] >= 0 and got[1] == 10, "%s: the Scw overload has no chi-square test, found %r" % (name, got)
        elif idx < 0:
            assert got == (-1, 256), "%s: meant to find nothing, found %r" % (name, got)
        else:
            assert got == (idx, dist), "%s: found %r, meant (%d, %d)" % (name, got, idx, dist)
            h = fuse_results[job][1]; h = h[h["cand"] == pos]
            if action:
                assert len(h) == 1 and int(h[0]["action"]) == action and int(h[0]["other"]) == (e[5] if len(e) > 5 else -1), "%s: hit %r" % (name, h)
    for name, (job, pos, idx, dist) in scene["expect_scw"].items():
        got = tuple(int(x) for x in fuse_results[job][0][pos])
        assert got == (idx, dist), "%s: found %r, meant (%d, %d)" % (name, got, idx, dist)


def wide_window_scene(cols):
    """One point whose window spans `cols` grid columns (16: one 16-lane group of the shared walk would do; 17: it would not), the
    nearest descriptor in the last column.  Level 7 (scale 3.583) and a column of 19.39 px: the radius is 0.18478 * th columns, and
    about u = 30.25 columns th = 39 opens columns 23 .. 38, th = 40 columns 22 .. 38.  th is integral: both functions take it."""
    th = {16: 39, 17: 40}[cols]
    S = SceneBuilder(700 + cols, th=float(th))
    A = S.keyframe(T1_DEFAULT)
    wi = fc.GRID_COLS / 1241.0
    lvl = 7
    u, v = 30.25 / wi, 200.0
    p = S.point(A, u, v, 10.0, lvl)
    rad = th * float(Levels().scale[lvl])
    for j, du in enumerate(np.linspace(-rad * 0.98, rad * 0.98, 40)):
        S.feature(A, u + du, v + (j % 5) - 2.0, p, 9 if j == 39 else 20 + j, octave=lvl)
    S.job(A, [p])
    sc = S.build("wide_%d" % cols)
    sc["th_proj"] = th
    return sc


def projection_scene():
    """What only SearchByProjection has: a candidate in spAlreadyFound, targets matched on entry (-2 and an index), and candidates that
    contend for features.  Each group sits at an anchor of its own (anchors are 80 px apart; th = 3 -> windows below 11 px).
    -> scene with expect {name: (position, bestIdx, bestDist, taken)}."""
    S = SceneBuilder(3)
    A = S.keyframe(T1_DEFAULT)
    rng = S.rng
    entries, ex, extra = [], {}, {}
    slot = [0]

    def anchor():
        i = slot[0]; slot[0] += 1
        return 80.0 + 80.0 * (i % 13), 40.0 + 60.0 * (i // 13)

    def cand(u, v, desc, name=None, want=None):
        p = S.point(A, u, v, 10.0, 2, desc=desc); entries.append(p)
        if name:
            ex[name] = (len(entries) - 1,) + want
        return p

    # already found: the candidate sits in vpMatched of some feature far away
    u, v = anchor(); fd = rand_desc(rng); f = S.kfs[A].add(u, v, fd, 2)
    p = cand(u, v, flipped(fd, 5, rng), "already_found", (-1, 256, False))
    far = S.kfs[A].add(1200.0, 350.0, rand_desc(rng), 2); extra[(0, far)] = p
    # target matched on entry: by a point outside the table (-2), by a point of the table
    for name, held in (("target_matched_outside", -2), ("target_matched_index", None)):
        u, v = anchor(); fd = rand_desc(rng); f = S.kfs[A].add(u, v, fd, 2)
        f2 = S.kfs[A].add(u + 1.0, v, flipped(fd, 60, rng), 2)
        other = S.point(A, 600.0, 5.0, 30.0, 2) if held is None else held
        extra[(0, f)] = other
        dsc = flipped(fd, 5, rng)
        cand(u, v, dsc, name, (f2, tc.hamming(dsc, S.kfs[A].desc[f2]), False))
    # two candidates on one feature; the loser has a second choice <= 50 / one > 50 / none
    for name, second in (("two_second_le50", 45), ("two_second_gt50", 55), ("two_none", None)):
        u, v = anchor(); fd = rand_desc(rng); f = S.kfs[A].add(u, v, fd, 2)
        a = flipped(fd, 10, rng); b = flipped(fd, 20, rng)
        g = S.kfs[A].add(u + 2.0, v, flipped(b, second, rng), 2) if second else -1
        if second:
            assert tc.hamming(a, S.kfs[A].desc[g]) > 10
        cand(u, v, a, name + "_winner", (f, 10, True))
        cand(u + 0.2, v, b, name + "_loser", (g, second if second else 256, bool(second and second <= TH_LOW)))
    # three candidates on one feature: the first takes it, the second takes its second choice, the third finds nothing
    u, v = anchor(); fd = rand_desc(rng); f = S.kfs[A].add(u, v, fd, 2)
    a, b, c = flipped(fd, 30, rng), flipped(fd, 5, rng), flipped(fd, 8, rng)
    g = S.kfs[A].add(u + 2.0, v, flipped(b, 40, rng), 2)
    assert tc.hamming(a, S.kfs[A].desc[g]) > 30 and tc.hamming(c, S.kfs[A].desc[g]) > 8
    cand(u, v, a, "three_first", (f, 30, True)); cand(u + 0.1, v, b, "three_second", (g, 40, True)); cand(u + 0.2, v, c, "three_third", (-1, 256, False))
    # a chain: A takes B's best, B takes C's best, C takes what is left
    u, v = anchor()
    f1d = rand_desc(rng); f2d = flipped(f1d, 40, rng); f3d = flipped(f2d, 40, rng)
    f1 = S.kfs[A].add(u, v, f1d, 2); f2 = S.kfs[A].add(u + 1.0, v, f2d, 2); f3 = S.kfs[A].add(u + 2.0, v, f3d, 2)
    da = flipped(f1d, 10, rng)
    db = _toward(f1d, f2d, 12, rng); dc = _toward(f2d, f3d, 14, rng)
    cand(u, v, da, "chain_a", (f1, 10, True)); cand(u + 0.1, v, db, "chain_b", (f2, tc.hamming(db, f2d), True))
    cand(u + 0.2, v, dc, "chain_c", (f3, tc.hamming(dc, f3d), True))
    assert tc.hamming(db, f1d) < tc.hamming(db, f2d) <= TH_LOW and tc.hamming(dc, f2d) < tc.hamming(dc, f3d) <= TH_LOW
    # pad so that the next contention straddles positions 63 / 64 of the list
    while len(entries) < 63:
        entries.append(-1)
    u, v = anchor(); fd = rand_desc(rng); f = S.kfs[A].add(u, v, fd, 2); g = S.kfs[A].add(u + 2.0, v, flipped(fd, 44, rng), 2)
    a = flipped(fd, 15, rng); b = flipped(fd, 3, rng)
    cand(u, v, a, "straddle_63", (f, 15, True))
    cand(u + 0.1, v, b, "straddle_64", (g, tc.hamming(b, S.kfs[A].desc[g]), tc.hamming(b, S.kfs[A].desc[g]) <= TH_LOW))
    assert ex["straddle_63"][0] == 63 and ex["straddle_64"][0] == 64
    # 65 candidates on one feature: the first takes it
    u, v = anchor(); fd = rand_desc(rng); f = S.kfs[A].add(u, v, fd, 2)
    for j in range(65):
        cand(u + 0.01 * j, v, flipped(fd, int(rng.integers(0, 40)), rng), "crowd_%d" % j if j in (0, 64) else None,
             (f, None, True) if j == 0 else (-1, 256, False))
    S.job(A, entries)
    sc = S.build("projection")
    sc["th_proj"] = 3
    sc = with_scale(sc, 1.0)
    sc["matched"] = matched_from_state(sc, extra)
    sc["expect_proj"] = ex
    return sc


def _toward(a, b, k, rng):
    """`a` with k of the bits flipped in which it differs from `b`: k from a, hamming(a, b) - k from b."""
    diff = np.nonzero(np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)))[0]
    return tc._flip(np.asarray(a, np.uint8), [(int(x) & ~7) | (7 - (int(x) & 7)) for x in rng.choice(diff, k, replace=False)])


def check_projection(scene, results):
    (assigned, best, nm), = results
    for name, (pos, idx, dist, taken) in scene["expect_proj"].items():
        got = tuple(int(x) for x in best[pos])
        assert got[0] == idx and (dist is None or got[1] == dist), "%s: found %r, meant (%r, %r)" % (name, got, idx, dist)
        assert (idx >= 0 and int(assigned[idx]) == pos) == taken, "%s: taken" % name


def random_scw_scene(seed, scale=None):
    """A random scene of fuse_cases.py under a similarity; the incoming vpMatched holds points outside the table where the feature state
    says so and a few candidates of the job's own list (spAlreadyFound)."""
    rng = np.random.default_rng(5100 + seed)
    sc = fc.random_scene(40 + seed, 4, 240, n_features=200, shared_list=seed % 2 == 0, noise=1.5)
    s = SCALES[seed % 4] if scale is None else scale
    sc = with_scale(sc, s)
    rows = matched_from_state(sc)
    for q, (k, entries, state) in enumerate(sc["jobs"]):
        occupied = np.nonzero(rows[q] == -2)[0]
        pick = rng.permutation(occupied)[:6]
        cands = entries[entries >= 0]
        rows[q][pick] = rng.choice(cands, len(pick), replace=False)
    sc["matched"] = rows
    sc["th"] = 4.0; sc["th_proj"] = 10
    return sc


def rigid_exact_scene(n_points=160, seed=0):
    """Scale 1 over a pose turned about the camera's x axis (row 0 of the rotation is (1, 0, 0): the decomposition returns the pose bit
    for bit).  Every feature lies on the projection of its point, mono and stereo mixed, at the predicted level or one below: all of
    them pass the chi-square test of Fuse(pKF, vpMapPoints, th), so that function and the Scw overload must agree."""
    rng = np.random.default_rng(5600 + seed)
    T = tc.pose(tc.rodrigues([0.05, 0.0, 0.0]), [0.3, -0.2, 0.5])
    S = SceneBuilder(800 + seed)
    A = S.keyframe(T)
    entries = []
    for q in range(n_points):
        u, v, z = 40.0 + 60.0 * (q % 20) + rng.uniform(0, 10), 25.0 + 40.0 * (q // 20) + rng.uniform(0, 10), rng.uniform(5, 40)
        level = int(rng.integers(1, 7))                          # cells of 60 x 40 px: no window (below 11 px) sees a neighbour's feature
        p = S.point(A, u, v, z, level); entries.append(p)
        if rng.random() < 0.85:
            S.feature(A, u, v, p, int(rng.integers(0, 71)), level - int(rng.integers(0, 2)), stereo_z=z if rng.random() < 0.5 else None)
    S.job(A, entries)
    sc = S.build("rigid_exact")
    sc["scw"] = [np.asarray(sc["kfs"][0]["Tcw"], F32).copy()]; sc["matched"] = [None]
    return sc


# ---------------------------------------------------------------- 1-ulp scans (Scw functions)
SCAN_KINDS = ("z", "u_min", "u_max", "v_min", "v_max", "dist_min", "dist_max", "view_angle", "window_x", "window_y")
SCAN_SCALE = 1.0          # scale 1 over an identity-row pose keeps the decomposition exact: the scans slide the projection, not Q41


def _scan_scene(kind, items):
    """One point and one feature per item (variant, sliding value).  The kinds fuse_cases.py has are its scenes; the others live on an
    identity pose: z slides the depth of a point on the optical axis through 0 (the camera sits at z = -2), the image bounds slide the
    abscissa / ordinate of a point at depth 1 whose projection crosses the bound."""
    if kind in fc.SCAN_KINDS:
        return with_scale(fc._scan_scene(kind, items), SCAN_SCALE)
    S = SceneBuilder(60 + SCAN_KINDS.index(kind))
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    if kind == "z":
        T = tc.pose(np.eye(3), [0.0, 0.0, 2.0])
        I = S.keyframe(T)
        entries = []
        for variant, val in items:
            r = np.zeros((), MP_DTYPE)
            r["xw"] = (0.0, 0.0, val); r["normal"] = (0.0, 0.0, 1.0); r["min_distance"] = 0.0; r["max_distance"] = 1.0; r["flags"] = 1
            S.points.append(r); S.pdesc.append(rand_desc(S.rng)); p = len(S.points) - 1
            S.kfs[I].add(float(cx) + 0.01 * variant, float(cy), flipped(S.pdesc[p], 10, S.rng), 7)       # max / dist is huge: the top level
            entries.append(p)
        S.job(I, entries)
        return with_scale(S.build("scan_z"), SCAN_SCALE)
    I = S.keyframe(np.eye(4))
    entries = []
    horizontal = kind in ("u_min", "u_max")
    inside = 10.0 if kind in ("u_min", "v_min") else -10.0        # a feature closer than 8 px to mnMaxX / mnMaxY falls outside the grid; level 7: radius 10.75
    target = {"u_min": CAM["mnMinX"], "u_max": CAM["mnMaxX"], "v_min": CAM["mnMinY"], "v_max": CAM["mnMaxY"]}[kind]
    for variant, val in items:
        other_px = 60.0 + 20.0 * variant
        if horizontal:
            X = [float(val), float((F32(other_px) - cy) / fy), 1.0]
        else:
            X = [float((F32(other_px * 3) - cx) / fx), float(val), 1.0]
        p = S.point_at(I, X, 7)
        if horizontal:
            S.feature(I, float(target) + inside, other_px, p, 10, octave=7)
        else:
            S.feature(I, other_px * 3, float(target) + inside, p, 10, octave=7)
        entries.append(p)
    S.job(I, entries)
    return with_scale(S.build("scan_" + kind), SCAN_SCALE)


def _scan_start(kind, variant):
    if kind in fc.SCAN_KINDS:
        return fc._scan_start(kind, variant)
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    if kind == "z":
        return None
    f, c = (fx, cx) if kind in ("u_min", "u_max") else (fy, cy)
    t = {"u_min": CAM["mnMinX"], "u_max": CAM["mnMaxX"], "v_min": CAM["mnMinY"], "v_max": CAM["mnMaxY"]}[kind]
    x = float((np.float64(t) - np.float64(c)) / np.float64(f))
    step = 2.0 / float(f)                                         # two pixels either side
    return (x + step, x - step) if kind in ("u_min", "v_min") else (x - step, x + step)


def scan_found(scene, contract="off"):
    """Per entry: the search found the entry's own feature (every other one is more than TH_LOW away)."""
    (best, hits, _), = cpu_fuse(scene, contract)[0]
    return best[:, 1] <= TH_LOW


def scan_scene(kind, steps=512):
    """`steps` entries in 16 windows of consecutive f32 values centred on the bound `kind` names; placed by bisection with the ORACLE."""
    W = fc.SCAN_WINDOWS
    per = steps // W

    def accepted(vals):
        return scan_found(_scan_scene(kind, list(enumerate(vals))))

    if kind == "z":
        # zc = z + 2 crosses 0 at z = -2 exactly (the sum is exact there): consecutive floats around -2, both signs of zc
        first = F32(-2.0).view(np.int32) - per // 2 + 1
        items = [(v, x) for v in range(W) for x in (first + np.arange(per)).astype(np.int32).view(F32)]
        return _scan_scene(kind, items)
    start = [_scan_start(kind, v) for v in range(W)]
    lo = np.array([s[0] for s in start], F32); hi = np.array([s[1] for s in start], F32)
    neg = bool(np.all(lo < 0) and np.all(hi < 0))
    assert neg or (np.all(lo > 0) and np.all(hi > 0)), "the bisection walks the integer view of floats of one sign"
    assert accepted(lo).all() and not accepted(hi).any(), kind
    li, hj = lo.view(np.int32).astype(np.int64), hi.view(np.int32).astype(np.int64)
    while np.any(np.abs(hj - li) > 1):
        mid = (li + hj) // 2
        ok = accepted(mid.astype(np.int32).view(F32))
        li, hj = np.where(ok, mid, li), np.where(ok, hj, mid)
    items = []
    for v in range(W):
        first = min(li[v], hj[v]) - per // 2 + 1
        items += [(v, x) for x in (first + np.arange(per)).astype(np.int32).view(F32)]
    return _scan_scene(kind, items)


# ---------------------------------------------------------------- keyframe-keyframe SearchByBoW
def cpu_bow(case, contract="off", twin="none"):
    """-> (match12 (N1,) [the side-2 twin: (max(N1, N2),)], nmatches, branches)"""
    L = oracle(contract)
    a, b = OracleKF(L, case["kf1"]), OracleKF(L, case["kf2"])
    L.sd_loop_oracle_reset_branches(); L.sd_loop_oracle_set_twin(TWINS[twin])
    n = max(a.N, b.N, 1)
    m = np.full(n, -1, np.int32)
    v1 = np.ascontiguousarray(case["valid1"], np.uint8) if case.get("valid1") is not None else None
    v2 = np.ascontiguousarray(case["valid2"], np.uint8) if case.get("valid2") is not None else None
    nm = L.sd_loop_oracle_bow(a.h, b.h, _p(v1), _p(v2), case.get("nnratio", 0.75), int(case.get("check_orientation", True)), _p(m))
    br = branches(L)
    L.sd_loop_oracle_set_twin(0)
    a.close(); b.close()
    return (m if twin == "bow_index_by_side2" else m[:a.N]).copy(), nm, br


def numpy_bow(case):
    """SearchByBoW restated: per shared node a distance matrix, rows in order, columns masked as they are taken."""
    k1, k2 = case["kf1"], case["kf2"]
    N1, N2 = len(k1["kp"]), len(k2["kp"])
    v1 = np.ones(N1, bool) if case.get("valid1") is None else np.asarray(case["valid1"][:N1], bool)
    v2 = np.ones(N2, bool) if case.get("valid2") is None else np.asarray(case["valid2"][:N2], bool)
    match = np.full(N1, -1, np.int32); bins = np.full(N1, -1, np.int64)
    ratio = F32(case.get("nnratio", 0.75))
    n1, f1 = k1["fv"]; n2, f2 = k2["fv"]
    for node in np.intersect1d(n1, n2):
        r1 = f1[n1 == node]; r2 = f2[n2 == node]
        free = v2[r2].copy()
        D = np.unpackbits(k1["desc"][r1][:, None, :] ^ k2["desc"][r2][None, :, :], axis=2).sum(2).astype(np.int64)
        for a, i1 in enumerate(r1):
            if not v1[i1] or not free.any():
                continue
            d = np.where(free, D[a], 1000)
            j = int(np.argmin(d)); d1 = int(d[j])
            if d1 >= 256:
                continue
            rest = np.delete(d, j)
            d2 = int(rest.min()) if len(rest) and rest.min() < 256 else 256
            if d1 < TH_LOW and F32(d1) < ratio * F32(d2):
                match[i1] = r2[j]; free[j] = False
                rot = F32(k1["kp"]["angle"][i1]) - F32(k2["kp"]["angle"][r2[j]])
                if rot < 0:
                    rot = F32(rot + F32(360.0))
                b = int(np.floor(F32(rot * (F32(1.0) / F32(HISTO))) + F32(0.5)))
                bins[i1] = 0 if b == HISTO else b
    if case.get("check_orientation", True):
        hist = np.bincount(bins[bins >= 0], minlength=HISTO)
        m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
        for i, s in enumerate(hist):
            if s > m1:
                m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
            elif s > m2:
                m3, m2, i3, i2 = m2, s, i2, i
            elif s > m3:
                m3, i3 = s, i
        if m2 < F32(0.1) * F32(m1):
            i2 = i3 = -1
        elif m3 < F32(0.1) * F32(m1):
            i3 = -1
        drop = (bins >= 0) & ~np.isin(bins, [i1, i2, i3])
        match[drop] = -1
    return match, int((match >= 0).sum())


class PairBuilder:
    """Two keyframes over the identities of one vocabulary.  kf1(slot, ident, d) adds a KF1 feature d bits from identity `ident` of
    node `slot`; likewise kf2."""

    def __init__(self, D, seed):
        self.D, self.rng = D, np.random.default_rng(8000 + seed)
        self.A, self.B = KeyFrameBuilder(T1_DEFAULT), KeyFrameBuilder(T1_DEFAULT)
        self.v1, self.v2 = [], []
        self.k = {}

    def ident(self, slot):
        self.k[slot] = self.k.get(slot, 0) + 1
        return self.D.identity(slot, self.k[slot] - 1)

    def _add(self, B, mask, desc, angle, valid):
        i = B.add(float(self.rng.uniform(20, 1200)), float(self.rng.uniform(10, 360)), desc, 0, angle)
        mask.append(1 if valid else 0)
        return i

    def kf1(self, desc, angle=0.0, valid=True):
        return self._add(self.A, self.v1, desc, angle, valid)

    def kf2(self, desc, angle=0.0, valid=True):
        return self._add(self.B, self.v2, desc, angle, valid)

    def near(self, ident, d):
        return self.D.candidate(ident, d)

    def build(self, name, voc_oracle, nnratio=0.75, check_orientation=True, **kw):
        k1, k2 = self.A.build(), self.B.build()
        tc.attach_bow([k1, k2], voc_oracle)
        c = dict(name=name, kf1=k1, kf2=k2, nnratio=nnratio, check_orientation=check_orientation,
                 valid1=None if all(self.v1) else np.array(self.v1, np.uint8), valid2=None if all(self.v2) else np.array(self.v2, np.uint8))
        c.update(kw)
        return c


def bow_cases(synth, voc_oracle, seed=5):
    """-> (vocabulary, {name: case}).  A case carries expect {idx1: idx2 or -1} for the features it was built around."""
    voc = tc.vocabulary(synth, seed)
    D = tc.Descriptors(voc, 900)
    cases = {}
    # ---- decision edges, one node each (orientation off: the histogram has a case of its own)
    P = PairBuilder(D, 1); ex = {}
    i = P.ident(0); a = P.kf1(i); b = P.kf2(P.near(i, 49)); ex[a] = b                               # 49 accepted
    i = P.ident(1); a = P.kf1(i); P.kf2(P.near(i, 50)); ex[a] = -1                                   # 50 rejected (the KF-Frame rule takes it)
    i = P.ident(2); a = P.kf1(i); b = P.kf2(P.near(i, 29)); P.kf2(P.near(i, 40)); ex[a] = b         # 29 < 0.75 * 40
    i = P.ident(3); a = P.kf1(i); P.kf2(P.near(i, 30)); P.kf2(P.near(i, 40)); ex[a] = -1            # 30 < 30 fails
    i = P.ident(4); a = P.kf1(i); b = P.kf2(P.near(i, 20)); ex[a] = b                                # a single side-2 feature: bestDist2 = 256
    i = P.ident(5); a = P.kf1(i, valid=False); P.kf2(P.near(i, 5)); ex[a] = -1                       # invalid side 1
    i = P.ident(6); a = P.kf1(i); P.kf2(P.near(i, 5), valid=False); b = P.kf2(P.near(i, 30)); ex[a] = b    # invalid side 2: the next one, alone
    P.kf1(P.ident(7))                                                                                # node 7 only in KF1
    P.kf2(P.ident(8))                                                                                # node 8 only in KF2
    i = P.ident(9); a = P.kf1(i); b = P.kf2(P.near(i, 12)); ex[a] = b                                # after both skips the walk goes on
    cases["edges"] = P.build("edges", voc_oracle, check_orientation=False, expect=ex)
    # ---- contention: two KF1 features prefer one KF2 feature
    P = PairBuilder(D, 2); ex = {}
    i = P.ident(0); f = P.kf2(i); a = P.kf1(P.near(i, 10)); bd = P.near(i, 20); b = P.kf1(bd)
    g = P.kf2(tc._flip(bd, P.rng.choice(256, 40, replace=False))); ex[a] = f; ex[b] = g              # the later takes its next best
    i = P.ident(1); f = P.kf2(i); a = P.kf1(P.near(i, 10)); bd = P.near(i, 20); b = P.kf1(bd)
    P.kf2(tc._flip(bd, P.rng.choice(256, 40, replace=False))); P.kf2(tc._flip(bd, P.rng.choice(256, 44, replace=False)))
    ex[a] = f; ex[b] = -1                                                                            # ... or fails the ratio (40 vs 44)
    cases["contention"] = P.build("contention", voc_oracle, nnratio=0.75, check_orientation=False, expect=ex)
    # equal distances: the earlier side-2 feature in the node's list wins (a tie fails every ratio below 1: nnratio 1.5 here)
    P = PairBuilder(D, 3); ex = {}
    i = P.ident(2); a = P.kf1(i); b1 = P.kf2(P.near(i, 15)); P.kf2(P.near(i, 15)); ex[a] = b1
    cases["tie"] = P.build("tie", voc_oracle, nnratio=1.5, check_orientation=False, expect=ex)
    # ---- node sizes on side 2: 64 / 65 / 128 / 129, and more than 64 KF1 features in a node
    for n2 in (64, 65, 128, 129):
        P = PairBuilder(D, 10 + n2); ex = {}
        ids = [P.ident(0) for _ in range(12)]
        for q in range(n2):                                      # the close ones last: they straddle positions 64 / 128 of the node's list
            P.kf2(P.near(ids[q % 12], int(P.rng.integers(38, 49)) if q < n2 - 12 else int(P.rng.integers(5, 13))))
        for q in range(12):
            P.kf1(P.near(ids[q], int(P.rng.integers(0, 8))))
        cases["node2_%d" % n2] = P.build("node2_%d" % n2, voc_oracle, nnratio=0.9, check_orientation=False, expect={})
    P = PairBuilder(D, 30)
    ids = [P.ident(0) for _ in range(20)]
    for q in range(70):
        P.kf1(P.near(ids[q % 20], int(P.rng.integers(0, 30))))
    for q in range(20):
        P.kf2(P.near(ids[q], int(P.rng.integers(0, 10))))
    cases["node1_70"] = P.build("node1_70", voc_oracle, nnratio=0.9, check_orientation=False, expect={})
    # ---- rotation: bin = round(rot / 30), so ORB angles (below 360) end in bins 0 .. 12 and `bin == HISTO_LENGTH` needs a difference of
    # 885 degrees or more: one key point carries the angle 899 to reach it.  11 matches at 0 degrees + the wrapped one, 12 at 120 and 12
    # at 354.5 (bin 12): three equal maxima; the one match at 240 degrees (bin 8) is removed.
    P = PairBuilder(D, 40); ex = {}
    plan = [(0.0, 0.0)] * 11 + [(899.0, 0.0)] + [(130.0, 10.0)] * 12 + [(357.0, 2.5)] * 12 + [(250.0, 10.0)]
    for q, (a1, a2) in enumerate(plan):
        i = P.ident(q % 10); a = P.kf1(i, angle=a1); b = P.kf2(P.near(i, 6), angle=a2)
        ex[a] = -1 if q == len(plan) - 1 else b
    cases["rotation"] = P.build("rotation", voc_oracle, nnratio=0.9, check_orientation=True, expect=ex)
    c = dict(cases["rotation"]); c["name"] = "rotation_off"; c["check_orientation"] = False
    c["expect"] = {a: (b if b >= 0 else len(plan) - 1) for a, b in ex.items()}
    cases["rotation_off"] = c
    # ---- an empty FeatureVector on either side
    P = PairBuilder(D, 50); P.kf1(P.ident(0))
    cases["empty_fv2"] = P.build("empty_fv2", voc_oracle, expect={0: -1})
    P = PairBuilder(D, 51); P.kf2(P.ident(0))
    cases["empty_fv1"] = P.build("empty_fv1", voc_oracle, expect={})
    return voc, cases


def random_bow_case(voc, voc_oracle, seed, n_points=260):
    """Two views of one scene of triangulate_cases.py with validity masks on both sides."""
    sc = tc.random_scene(voc, 60 + seed, n_points, 1)
    rng = np.random.default_rng(8800 + seed)
    k1, k2 = sc["kf1"], sc["neighbours"][0]
    tc.attach_bow([k1, k2], voc_oracle)
    return dict(name="random_bow_%d" % seed, kf1=k1, kf2=k2, nnratio=0.75 if seed % 2 else 0.9, check_orientation=seed % 3 != 0,
                valid1=(rng.random(len(k1["kp"])) < 0.85).astype(np.uint8), valid2=(rng.random(len(k2["kp"])) < 0.85).astype(np.uint8), expect={})


# ---------------------------------------------------------------- the device side (tests marked gpu, tools)
Workspace = fc.Workspace


def _tables(scene):
    import torch
    jobs = scene["jobs"]
    off = np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int32)
    ent = np.concatenate([j[1] for j in jobs] + [np.zeros(0, np.int32)]).astype(np.int32)
    pts = np.ascontiguousarray(scene["points"], MP_DTYPE)
    d_ent = torch.from_numpy(ent).cuda() if len(ent) else None
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda() if len(pts) else None
    d_desc = torch.from_numpy(np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1).copy()).cuda() if len(pts) else None
    S = np.array(scene["scw"], F32).reshape(len(jobs), 16) if jobs else np.zeros((0, 16), F32)
    return off, d_ent, d_pts, d_desc, S, len(pts)


def device_fuse(ws, scene, cam=CAM, upload=True):
    """One sd_batch_fuse_sim3 for all jobs of the scene -> [(best, hits, nfused)]."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    jobs = scene["jobs"]
    off, d_ent, d_pts, d_desc, S, npts = _tables(scene)
    d_state = None
    if any(j[2] is not None for j in jobs):
        st = np.zeros((len(jobs), ws.cap), np.uint8)
        for q, j in enumerate(jobs):
            if j[2] is not None:
                st[q, :len(j[2])] = j[2]
        d_state = torch.from_numpy(st).cuda()
    ptr = lambda t: t.data_ptr() if t is not None else None
    ws.b.fuse_sim3([j[0] for j in jobs], S, off, ptr(d_ent), ptr(d_pts), ptr(d_desc), cam, th=scene.get("th", 3.0), d_kf_state=ptr(d_state), n_points=npts)
    out = [ws.b.download_fuse(q) for q in range(len(jobs))]
    del d_ent, d_pts, d_desc, d_state
    return out


def device_project(ws, scene, cam=CAM, upload=True):
    """One sd_batch_search_by_projection_sim3 for all jobs -> [(assigned (cap,), best, nmatches)]."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    jobs = scene["jobs"]
    off, d_ent, d_pts, d_desc, S, npts = _tables(scene)
    m = np.full((max(len(jobs), 1), ws.cap), -1, np.int32)
    for q, row in enumerate(scene["matched"]):
        if row is not None:
            m[q, :len(row)] = row
    d_m = torch.from_numpy(m).cuda()
    ptr = lambda t: t.data_ptr() if t is not None else None
    ws.b.search_by_projection_sim3([j[0] for j in jobs], S, off, ptr(d_ent), ptr(d_pts), ptr(d_desc), d_m.data_ptr(), cam,
                                   th=int(scene.get("th_proj", 10)), n_points=npts)
    out = [ws.b.download_projection_sim3(q) for q in range(len(jobs))]
    del d_ent, d_pts, d_desc, d_m
    return out


def device_bow(ws, cases):
    """All cases in one sd_batch_search_by_bow_kf (two slots per case) -> [(match12 (N1,), nmatches)]."""
    import torch
    kfs = [k for c in cases for k in (c["kf1"], c["kf2"])]
    ws.upload(kfs)
    n = len(cases)
    v1 = np.ones((n, ws.cap), np.uint8); v2 = np.ones((n, ws.cap), np.uint8)
    for q, c in enumerate(cases):
        if c.get("valid1") is not None:
            v1[q, :len(c["valid1"])] = c["valid1"]
        if c.get("valid2") is not None:
            v2[q, :len(c["valid2"])] = c["valid2"]
    d1, d2 = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    ratios = set((c.get("nnratio", 0.75), bool(c.get("check_orientation", True))) for c in cases)
    assert len(ratios) == 1, "one call has one nnratio and one orientation switch"
    (ratio, ori), = ratios
    ws.b.search_by_bow_kf(list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)), ratio, ori, d1.data_ptr(), d2.data_ptr())
    out = []
    for q, c in enumerate(cases):
        match, pairs, nm = ws.b.download_matches(q)
        assert len(pairs) == 0 and np.all(match[len(c["kf1"]["kp"]):] == -1)
        out.append((match[:len(c["kf1"]["kp"])].copy(), nm))
    del d1, d2
    return out


def assert_same_project(scene, got, want):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s job %d: nmatches %d vs %d" % (scene["name"], q, g[2], w[2])
        assert g[1].tobytes() == w[1].tobytes(), "%s job %d: best differs at entries %r" % (scene["name"], q, np.nonzero((g[1] != w[1]).any(1))[0][:8])
        n = len(w[0])
        assert g[0][:n].tobytes() == w[0].tobytes() and np.all(g[0][n:] == -1), "%s job %d: assigned differs" % (scene["name"], q)
