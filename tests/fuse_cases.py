"""Shared by test_fuse_oracle.py, test_gpu_fuse.py, tools/fuzz_fuse.py and tools/bench_fuse.py: the ORBmatcher::Fuse /
ComputeDistinctiveDescriptors CPU oracle (tests/cpp/fuse_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary
directory) and seeded crafted scenes in plain numpy.

A scene is dict(kfs [keyframe dicts of KeyFrameBuilder.build()], points (MP_DTYPE), pdesc (n, 32) u8, jobs [(keyframe, entries i32,
state u8 [N] or None)], th, expect {name: (job, position, bestIdx or -1, bestDist or None, action or None)}).  A job is one call
Fuse(pKF, vpMapPoints, th); an entry indexes `points` or is -1.  The device tests write the keyframes over workspace slots, run
sd_batch_assign_grid and one sd_batch_fuse for all jobs; the CPU side runs the sequential oracle per job.
Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import triangulate_cases as tc
from triangulate_cases import CAM, F32, KP_DTYPE, KeyFrameBuilder, Levels, T1_DEFAULT, _p, pose, project, rodrigues, to_world

ROOT = tc.ROOT
MP_DTYPE = np.dtype([("xw", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("flags", "<u4")])
HIT_DTYPE = np.dtype([("cand", "<i4"), ("idx", "<i4"), ("dist", "<i4"), ("action", "<i4"), ("other", "<i4")])
ADD, MEET_KF, MEET_BAD, MEET_CANDIDATE = 1, 2, 3, 4
BRANCHES = ["entry_skip", "searched", "z_negative", "z_zero", "out_of_image", "u_eq_maxx", "u_eq_minx", "dist_below_min", "dist_above_max",
            "view_angle", "window_empty", "clip_left", "clip_right", "clip_top", "clip_bottom", "octave_below", "octave_above", "octave_lm1",
            "octave_l", "stereo_fail", "stereo_pass", "mono_fail", "mono_pass", "uright_zero_stereo", "tie_earlier_wins",
            "tie_higher_index_earlier", "closer_out_of_range", "dist50", "dist51", "meet_kf", "meet_bad", "add", "meet_candidate",
            "no_features", "empty_job", "window_over_64"]
GRID_COLS, GRID_ROWS = 64, 48
IDENTITY = np.eye(4)

_oracles = {}


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast (to count the decisions that changes)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="fuse_oracle_")
        so = os.path.join(d, "libfuse_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []          # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "fuse_oracle.cpp")])
        L = C.CDLL(so)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.sd_fuse_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_fuse_oracle_kf_new.restype = vp
        L.sd_fuse_oracle_kf_new.argtypes = [i, vp, vp, vp, vp, vp, i, vp, vp]
        L.sd_fuse_oracle_kf_free.argtypes = [vp]
        L.sd_fuse_oracle_search.argtypes = [vp, vp, vp, f, vp]
        L.sd_fuse_oracle_job.argtypes = [vp, i, vp, vp, vp, vp, f, vp, vp, vp]
        L.sd_fuse_oracle_distinctive.argtypes = [i, vp, vp]
        L.sd_fuse_model_new.restype = vp
        L.sd_fuse_model_free.argtypes = [vp]
        L.sd_fuse_model_add_kf.argtypes = [vp, vp]
        L.sd_fuse_model_add_point.argtypes = [vp, vp, vp, i]
        L.sd_fuse_model_observe.argtypes = [vp, i, i, i]
        L.sd_fuse_model_set_feature.argtypes = [vp, i, i, i]
        L.sd_fuse_model_fuse.argtypes = [vp, i, i, vp, f]
        L.sd_fuse_model_snapshot.argtypes = [vp, i, i, vp, vp, vp]
        L.sd_fuse_model_search.argtypes = [vp, i, i, vp, f, vp]
        L.sd_fuse_model_tail.argtypes = [vp, i, i, vp, vp]
        L.sd_fuse_model_point_count.argtypes = [vp]
        L.sd_fuse_model_points.argtypes = [vp, vp, vp, vp, vp]
        L.sd_fuse_model_dump.argtypes = [vp, vp, i]
        assert L.sd_fuse_oracle_branch_count() == len(BRANCHES)
        _oracles[contract] = L
    return _oracles[contract]


def branches(L, reset=False):
    b = L.sd_fuse_oracle_branches()
    out = {name: int(b[i]) for i, name in enumerate(BRANCHES)}
    if reset:
        L.sd_fuse_oracle_reset_branches()
    return out


def cam_array(cam=CAM):
    return np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")], F32)


def inv_sigma2(lv):
    """mvInvLevelSigma2 (ORBextractor.cc:428-429): 1.0f / mvLevelSigma2[i]."""
    return (F32(1) / lv.sigma2).astype(F32)


class OracleKF:
    """A keyframe of the oracle: key points, descriptors, uRight, pose, the 64 x 48 grid."""

    def __init__(self, L, kf, cam=CAM, lv=None):
        lv = lv or Levels()
        self.L, self.N = L, len(kf["kp"])
        kp = np.ascontiguousarray(kf["kp"], KP_DTYPE); d = np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1); ur = np.ascontiguousarray(kf["ur"], F32)
        T = np.ascontiguousarray(kf["Tcw"], F32).reshape(16); c = cam_array(cam); iv = inv_sigma2(lv)
        self.h = L.sd_fuse_oracle_kf_new(self.N, _p(kp), _p(d), _p(ur), _p(T), _p(c), lv.nlevels, _p(lv.scale), _p(iv))
        self.owned = True

    def close(self):
        if self.owned and self.h:
            self.L.sd_fuse_oracle_kf_free(self.h)
        self.h = None


def run_job(L, okf, entries, points, pdesc, state, th):
    """The sequential oracle on one job -> (best (n, 2) i32, hits (HIT_DTYPE), nfused)."""
    n = len(entries)
    e = np.ascontiguousarray(entries, np.int32); p = np.ascontiguousarray(points, MP_DTYPE); d = np.ascontiguousarray(pdesc, np.uint8).reshape(-1)
    best = np.zeros((max(n, 1), 2), np.int32); hits = np.zeros(max(n, 1), HIT_DTYPE); nh = np.zeros(1, np.int32)
    st = np.ascontiguousarray(state, np.uint8) if state is not None else None
    assert st is None or len(st) >= okf.N
    nf = L.sd_fuse_oracle_job(okf.h, n, _p(e), _p(p), _p(d), _p(st) if st is not None else None, th, _p(best), _p(hits), _p(nh))
    assert nf == nh[0]
    return best[:n].copy(), hits[:nh[0]].copy(), nf


def cpu_run(scene, contract="off", cam=CAM, lv=None):
    """Every job of a scene through the sequential oracle -> ([(best, hits, nfused)], branches)."""
    L = oracle(contract)
    okfs = [OracleKF(L, k, cam, lv) for k in scene["kfs"]]
    L.sd_fuse_oracle_reset_branches()
    out = []
    for k, entries, state in scene["jobs"]:
        out.append(run_job(L, okfs[k], entries, scene["points"], scene["pdesc"], state, scene.get("th", 3.0)))
    br = branches(L)
    for o in okfs:
        o.close()
    return out, br


def distinctive(descs, contract="off"):
    """ComputeDistinctiveDescriptors on vDescriptors (N, 32) -> (BestIdx or -1, descriptor or None)."""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    out = np.zeros(32, np.uint8)
    b = oracle(contract).sd_fuse_oracle_distinctive(len(d), _p(d) if len(d) else None, _p(out))
    return b, (out if b >= 0 else None)


def distinctive_numpy(descs):
    """The same rule restated in numpy: full matrix, zero diagonal, rows sorted, element (N - 1) // 2, the first strictly smallest."""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    if not len(d):
        return -1
    D = np.unpackbits(d[:, None, :] ^ d[None, :, :], axis=2).sum(2)
    med = np.sort(D, axis=1)[:, (len(d) - 1) // 2]
    return int(np.argmin(med))


# ---------------------------------------------------------------- the map model (c)
class Model:
    """Points with observation maps, keyframes with mvpMapPoints: runs the literal Fuse including Replace / AddObservation."""

    def __init__(self, kfs, cam=CAM, lv=None, contract="off"):
        self.L = oracle(contract)
        self.h = self.L.sd_fuse_model_new()
        self.kfs = kfs
        for k in kfs:
            o = OracleKF(self.L, k, cam, lv)
            self.L.sd_fuse_model_add_kf(self.h, o.h)
            o.owned = False

    def close(self):
        self.L.sd_fuse_model_free(self.h)

    def add_point(self, rec, desc, bad=False):
        r = np.ascontiguousarray(rec, MP_DTYPE).reshape(1); d = np.ascontiguousarray(desc, np.uint8)
        return self.L.sd_fuse_model_add_point(self.h, _p(r), _p(d), int(bad))

    def observe(self, p, kf, idx):
        self.L.sd_fuse_model_observe(self.h, p, kf, idx)

    def set_feature(self, kf, idx, p):
        self.L.sd_fuse_model_set_feature(self.h, kf, idx, p)

    def fuse(self, kf, cand, th=3.0):
        c = np.ascontiguousarray(cand, np.int32)
        return self.L.sd_fuse_model_fuse(self.h, kf, len(c), _p(c), th)

    def snapshot(self, kf, cand):
        """-> (entries i32 with -1 where the reference `continue`s, state u8 [N])"""
        c = np.ascontiguousarray(cand, np.int32); e = np.zeros(max(len(c), 1), np.int32); s = np.zeros(max(len(self.kfs[kf]["kp"]), 1), np.uint8)
        self.L.sd_fuse_model_snapshot(self.h, kf, len(c), _p(c), _p(e), _p(s))
        return e[:len(c)].copy(), s[:len(self.kfs[kf]["kp"])].copy()

    def search(self, kf, cand, th=3.0):
        c = np.ascontiguousarray(cand, np.int32); best = np.zeros((max(len(c), 1), 2), np.int32)
        self.L.sd_fuse_model_search(self.h, kf, len(c), _p(c), th, _p(best))
        return best[:len(c)].copy()

    def tail(self, kf, cand, best):
        c = np.ascontiguousarray(cand, np.int32); b = np.ascontiguousarray(best, np.int32)
        return self.L.sd_fuse_model_tail(self.h, kf, len(c), _p(c), _p(b))

    def points(self):
        """-> (records MP_DTYPE, descriptors (n, 32), bad u8, Observations() i32) of every point as the model stands"""
        n = self.L.sd_fuse_model_point_count(self.h)
        r = np.zeros(max(n, 1), MP_DTYPE); d = np.zeros((max(n, 1), 32), np.uint8); b = np.zeros(max(n, 1), np.uint8); o = np.zeros(max(n, 1), np.int32)
        self.L.sd_fuse_model_points(self.h, _p(r), _p(d), _p(b), _p(o))
        return r[:n], d[:n], b[:n], o[:n]

    def dump(self):
        n = self.L.sd_fuse_model_dump(self.h, None, 0)
        out = np.zeros(n, np.uint8)
        self.L.sd_fuse_model_dump(self.h, _p(out), n)
        return out.tobytes()


# ---------------------------------------------------------------- geometry and descriptors
def rand_desc(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8)


def flipped(desc, d, rng):
    """`desc` with exactly d bits flipped."""
    return tc._flip(np.asarray(desc, np.uint8), rng.choice(256, d, replace=False))


def cell_of(x, y, cam=CAM):
    """Frame::PosInGrid in f32 -> (column, row) or None."""
    wi = F32(GRID_COLS) / (cam["mnMaxX"] - cam["mnMinX"]); hi = F32(GRID_ROWS) / (cam["mnMaxY"] - cam["mnMinY"])
    px = int(np.round((F32(x) - cam["mnMinX"]) * wi)); py = int(np.round((F32(y) - cam["mnMinY"]) * hi))
    return (px, py) if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS else None


def centre(T):
    return to_world(T, [0.0, 0.0, 0.0])[0]


def point_record(T, Xw, level=0, lv=None, normal=None, min_distance=None, max_distance=None):
    """A map point at Xw that keyframe T predicts at `level`: the normal looks at the camera centre, mfMaxDistance sits half a level
    above the distance (PredictScale = ceil(log(max / dist) / log(1.2))), mfMinDistance = mfMaxDistance / scale[nlevels - 1]."""
    lv = lv or Levels()
    po = np.asarray(Xw, np.float64) - centre(T); dist = np.linalg.norm(po)
    r = np.zeros((), MP_DTYPE)
    r["xw"] = Xw
    r["normal"] = (po / dist) if normal is None else normal
    mx = dist * float(lv.scale_factor) ** (level - 0.5) if max_distance is None else max_distance
    r["max_distance"] = mx
    r["min_distance"] = mx / float(lv.scale[-1]) if min_distance is None else min_distance
    r["flags"] = 1
    return r


class SceneBuilder:
    def __init__(self, seed, th=3.0, lv=None):
        self.rng = np.random.default_rng(9000 + seed)
        self.lv = lv or Levels()
        self.kfs, self.poses, self.points, self.pdesc, self.jobs, self.expect, self.th = [], [], [], [], [], {}, th

    def keyframe(self, T=T1_DEFAULT):
        self.kfs.append(KeyFrameBuilder(T)); self.poses.append(np.asarray(T, np.float64))
        return len(self.kfs) - 1

    def point(self, k, u, v, z, level=2, desc=None, **kw):
        """A point that keyframe k sees at pixel (u, v), depth z -> its index."""
        X = tc.from_pixel(self.poses[k], u, v, z)
        return self.point_at(k, X, level, desc, **kw)

    def point_at(self, k, X, level=2, desc=None, **kw):
        self.points.append(point_record(self.poses[k], X, level, self.lv, **kw))
        self.pdesc.append(rand_desc(self.rng) if desc is None else np.asarray(desc, np.uint8))
        return len(self.points) - 1

    def feature(self, k, u, v, p=None, d=10, octave=2, desc=None, **kw):
        """A feature of keyframe k at (u, v) whose descriptor is d bits from point p's."""
        ds = flipped(self.pdesc[p], d, self.rng) if desc is None else desc
        return self.kfs[k].add(u, v, ds, octave, **kw)

    def job(self, k, entries, state=None):
        self.jobs.append((k, np.asarray(entries, np.int32), state))
        return len(self.jobs) - 1

    def build(self, name="scene"):
        pts = np.array(self.points, MP_DTYPE) if self.points else np.zeros(0, MP_DTYPE)
        return dict(name=name, kfs=[k.build() for k in self.kfs], points=pts, pdesc=np.array(self.pdesc, np.uint8).reshape(len(pts), 32),
                    jobs=[(j[0], j[1], None if j[2] is None else np.asarray(j[2], np.uint8)) for j in self.jobs], th=self.th,
                    expect=self.expect)


def solve_px(target, f, c):
    """x (f32) with fl(fl(f * x) + c) == target, as the projection computes u at depth 1 under the identity pose."""
    x0 = F32((np.float64(target) - np.float64(c)) / np.float64(f))
    xs = (x0.view(np.int32) + np.arange(-4000, 4001, dtype=np.int32)).astype(np.int32).view(F32)
    u = (F32(f) * xs).astype(F32) + F32(c)
    ok = np.nonzero(u.astype(F32) == F32(target))[0]
    assert len(ok), "no f32 abscissa projects onto %r" % target
    return xs[ok[len(ok) // 2]]


# ---------------------------------------------------------------- crafted cases
def crafted_scene():
    """Every branch of the search and of the resolve step, one anchor each.  Job 0: keyframe A (the usual pose), with feature states;
    job 1: keyframe I (identity pose, points at depth 1: exact image bounds); job 2: keyframe E without features; job 3: an empty job."""
    S = SceneBuilder(1)
    A = S.keyframe(T1_DEFAULT)
    rng = S.rng
    entries, state, ex = [], {}, S.expect
    slot = [0]

    def anchor():
        """Anchors 70 px apart horizontally, 45 px vertically: no window (radius < 11 px) sees a neighbour's features."""
        i = slot[0]; slot[0] += 1
        return 80.0 + 70.0 * (i % 15), 40.0 + 45.0 * (i // 15)

    def single(name, d=10, octave=2, level=2, off=(0.0, 0.0), st=None, want_hit=True, **fkw):
        u, v = anchor()
        p = S.point(A, u, v, 10.0, level)
        f = S.feature(A, u + off[0], v + off[1], p, d, octave, **fkw)
        entries.append(p)
        if st is not None:
            state[f] = st
        ex[name] = (0, len(entries) - 1, f if want_hit is not None else -1, d if want_hit is not None else None, want_hit)
        return p, f

    single("d50", d=50, want_hit=ADD)
    single("d51", d=51, want_hit=0)                       # found (bestDist 51) but not fused
    # a tie at distance 20: the feature added later (the higher index) lies one grid column to the left, is visited first and wins
    wi = float(GRID_COLS) / 1241.0
    u, v = (10 + 0.5) / wi, 200.0                        # on the border between columns 10 and 11
    p = S.point(A, u, v, 10.0, 2)
    f_lo = S.feature(A, u + 3.0, v, p, 20)
    f_hi = S.feature(A, u - 3.0, v, p, 20)
    assert cell_of(u - 3.0, v)[0] < cell_of(u + 3.0, v)[0] and f_hi > f_lo
    entries.append(p); ex["tie"] = (0, len(entries) - 1, f_hi, 20, ADD)
    # a closer feature two levels off loses to a farther one in range
    u, v = anchor(); p = S.point(A, u, v, 10.0, 3)
    S.feature(A, u + 1.0, v, p, 5, octave=1)
    f = S.feature(A, u - 1.0, v, p, 30, octave=3)
    entries.append(p); ex["closer_out_of_range"] = (0, len(entries) - 1, f, 30, ADD)
    single("octave_lm1", octave=1, level=2, want_hit=ADD)
    single("octave_l", octave=2, level=2, want_hit=ADD)
    single("octave_lp1", octave=3, level=2, want_hit=None)
    # chi-square: level 0, sigma2 = 1, radius 3.  ex = ey = 1.5: 4.5 passes 5.99; with er = 2 the stereo sum 8.5 fails 7.8
    for name, stereo, off, hit in (("stereo_fails", True, (1.5, 1.5), None), ("same_offsets_mono", False, (1.5, 1.5), ADD),
                                   ("mono_fails", False, (2.0, 2.0), None), ("stereo_passes", True, (0.5, 0.5), ADD)):
        u, v = anchor(); p = S.point(A, u, v, 10.0, 0)
        ur = float(F32(u) - CAM["mbf"] / F32(10.0))
        f = S.feature(A, u + off[0], v + off[1], p, 10, octave=0, ur=(ur - 2.0 if name == "stereo_fails" else ur) if stereo else None)
        entries.append(p); ex[name] = (0, len(entries) - 1, f if hit else -1, 10 if hit else None, hit)
    # uRight == 0 is a stereo feature (>= 0): er is the whole projected uRight, the test fails; as a mono feature it would pass
    single("uright_zero", octave=0, level=0, ur=0.0, want_hit=None)
    # behind the camera
    entries.append(S.point_at(A, to_world(T1_DEFAULT, [0.5, 0.2, -4.0])[0], 2)); ex["z_negative"] = (0, len(entries) - 1, -1, None, None)
    # image borders clip the window: right (columns beyond 63), bottom (rows beyond 47), top
    for name, (u, v) in (("clip_right", (1229.0, 150.0)), ("clip_bottom", (640.0, 366.0)), ("clip_top", (700.0, 2.5))):
        p = S.point(A, u, v, 10.0, 2); f = S.feature(A, u - 1.0, v, p, 10)
        assert cell_of(u - 1.0, v) is not None
        entries.append(p); ex[name] = (0, len(entries) - 1, f, 10, ADD)
    # nothing near
    u, v = anchor(); entries.append(S.point(A, u, v, 10.0, 2)); ex["empty_window"] = (0, len(entries) - 1, -1, None, None)
    # dist3D on either side of 0.8 * mfMinDistance and 1.2 * mfMaxDistance (1 % away)
    for name, q, which, hit in (("below_min", 0.79, "min", None), ("above_min", 0.81, "min", ADD), ("above_max", 1.21, "max", None),
                                ("below_max", 1.19, "max", ADD)):
        u, v = anchor(); X = tc.from_pixel(T1_DEFAULT, u, v, 10.0); dist = np.linalg.norm(X - centre(T1_DEFAULT))
        kw = dict(min_distance=dist / q) if which == "min" else dict(max_distance=dist / q, min_distance=dist / 8)
        lvl = 2 if which == "min" else 0
        p = S.point_at(A, X, lvl, **kw); f = S.feature(A, u, v, p, 10, octave=lvl)
        entries.append(p); ex[name] = (0, len(entries) - 1, f if hit else -1, 10 if hit else None, hit)
    # the viewing angle: the normal 61 / 59 degrees off the viewing ray
    for name, deg, hit in (("angle_61", 61.0, None), ("angle_59", 59.0, ADD)):
        u, v = anchor(); X = tc.from_pixel(T1_DEFAULT, u, v, 10.0); po = X - centre(T1_DEFAULT); po /= np.linalg.norm(po)
        side = np.cross(po, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
        n = np.cos(np.radians(deg)) * po + np.sin(np.radians(deg)) * side
        p = S.point_at(A, X, 2, normal=n); f = S.feature(A, u, v, p, 10)
        entries.append(p); ex[name] = (0, len(entries) - 1, f if hit else -1, 10 if hit else None, hit)
    # outside the image
    entries.append(S.point(A, -50.0, 100.0, 10.0, 2)); ex["out_of_image"] = (0, len(entries) - 1, -1, None, None)
    # a window of 66 features (a second pass of the device's wave); the nearest descriptor comes late in the walk
    u, v = 500.0, 300.0; p = S.point(A, u, v, 10.0, 2)
    for j in range(66):
        f = S.feature(A, u + rng.uniform(-2, 2), v + rng.uniform(-2, 2), p, 11 if j == 60 else int(rng.integers(13, 60)))
        if j == 60:
            f_best = f
    entries.append(p); ex["window_66"] = (0, len(entries) - 1, f_best, 11, ADD)
    # a -1 entry
    entries.append(-1); ex["skipped"] = (0, len(entries) - 1, -1, None, None)
    # what the feature holds
    single("meet_kf", st=1, want_hit=MEET_KF)
    single("meet_bad", st=2, want_hit=MEET_BAD)
    # two and three entries on one empty feature: the first adds, the others meet it
    for name, n in (("two_on_one", 2), ("three_on_one", 3)):
        u, v = anchor(); fd = rand_desc(rng)
        f = S.kfs[A].add(u, v, fd, 2)
        first = len(entries)
        for j in range(n):
            entries.append(S.point(A, u + 0.3 * j, v, 10.0 + j, 2, desc=flipped(fd, 10 + 10 * (n - j), rng)))
            ex["%s_%d" % (name, j)] = (0, len(entries) - 1, f, 10 + 10 * (n - j), ADD if j == 0 else MEET_CANDIDATE, -1 if j == 0 else first)
    nA = len(S.kfs[A].rows)
    st = np.zeros(nA, np.uint8)
    for f, s in state.items():
        st[f] = s
    S.job(A, entries, st)
    # keyframe I: identity pose, points at depth 1, so u = fl(fl(fx * x) + cx) exactly
    I = S.keyframe(IDENTITY)
    eI = []
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    y_mid = float((F32(150.0) - cy) / fy)
    for name, target, hit in (("u_eq_maxx", CAM["mnMaxX"], None), ("u_eq_minx", CAM["mnMinX"], ADD)):
        x = solve_px(target, fx, cx)
        p = S.point_at(I, [float(x), y_mid, 1.0], 2); f = S.feature(I, float(target) + (1.0 if hit else -1.0), 150.0, p, 10)
        eI.append(p); ex[name] = (1, len(eI) - 1, f if hit else -1, 10 if hit else None, hit)
    # zc == 0: u is not finite, IsInImage rejects it
    p = S.point_at(I, [0.3, 0.1, 1.0], 2); S.points[p]["xw"] = (0.3, 0.1, 0.0); eI.append(p); ex["z_zero"] = (1, len(eI) - 1, -1, None, None)
    S.job(I, eI)
    # keyframe E: N = 0
    E = S.keyframe(T1_DEFAULT)
    S.job(E, [S.point(E, 300.0, 200.0, 10.0, 2)]); ex["no_features"] = (2, 0, -1, None, None)
    S.job(A, [])
    return S.build("crafted")


def check_expectations(scene, results):
    """The crafted anchors found what they were built to find."""
    for name, e in scene["expect"].items():
        job, pos, idx, dist, action = e[:5]
        best, hits, _ = results[job]
        got = tuple(int(x) for x in best[pos])
        if idx < 0:
            assert got == (-1, 256), "%s: meant to find nothing, found %r" % (name, got)
            continue
        assert got == (idx, dist), "%s: found %r, meant (%d, %d)" % (name, got, idx, dist)
        h = hits[hits["cand"] == pos]
        if action:
            assert len(h) == 1 and int(h[0]["action"]) == action and int(h[0]["idx"]) == idx and int(h[0]["dist"]) == dist, "%s: hit %r" % (name, h)
            assert int(h[0]["other"]) == (e[5] if len(e) > 5 else -1), "%s: other %r" % (name, h)
        else:
            assert len(h) == 0, "%s: not meant to fuse" % name


# ---------------------------------------------------------------- 1-ulp scans
SCAN_KINDS = ("chi2_mono", "chi2_stereo", "dist_min", "dist_max", "view_angle", "window_x", "window_y")
SCAN_WINDOWS = 16
SCAN_TH = {"window_x": 2.0, "window_y": 2.0}       # with th = 3 the chi-square bound lies inside the window: the window never decides


def _scan_geometry(kind, variant):
    """Where the items of window `variant` project: (u, v, z).  The kinds that slide an image coordinate sit at a border."""
    small = 0.05 + 0.11 * variant
    z = 10.0 + 0.9 * variant
    if kind == "chi2_mono":
        return 100.0 + 60.0 * variant, small + 2.4, z
    if kind == "window_y":
        return 100.0 + 60.0 * variant, small + 2.0, z
    if kind == "window_x":
        return small + 2.0, 15.0 + 22.0 * variant, z
    if kind == "chi2_stereo":
        return small + 2.8 + float(CAM["mbf"]) / z, 15.0 + 22.0 * variant, z
    return 100.0 + 60.0 * variant, 100.0 + 50.0 * (variant % 4), z


def _scan_normal(X):
    """A normal 60 degrees off the viewing ray of X (the dot product sits on the bound), turned about the image's vertical."""
    po = X - centre(T1_DEFAULT); po /= np.linalg.norm(po)
    side = np.cross(po, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
    if side[2] < 0:
        side = -side                                     # towards +z: the component the scan slides stays well above 0
    return 0.5 * po + np.sqrt(0.75) * side


def _scan_scene(kind, items):
    """One point and one feature of its own per item (geometry variant, sliding value); the items of a variant share the projection,
    and random descriptors keep every feature but an item's own more than TH_LOW away, so an item fuses iff its own feature passes.
    Level 0 (sigma2 = 1) where an image coordinate slides.  What slides:
    chi2_mono    kp.y of a mono feature above the projection (u - kp.x = 0.5): 5.99
    chi2_stereo  uRight of a stereo feature at the projection: 7.8
    dist_min     mfMinDistance; dist_max: mfMaxDistance (the raw values: the products 0.8f * / 1.2f * are part of the bound)
    view_angle   the z component of a normal 60 degrees off the viewing ray
    window_x     kp.x left of the projection, kp.y on it, th = 2: |distx| < r; window_y: the same for kp.y
    The sliding image coordinates lie within a few pixels of 0, where one f32 step moves the squared error by less than one of ITS
    ulps: the scan resolves the bound to the last bit, and a contraction (which moves the error by one ulp) flips decisions."""
    S = SceneBuilder(50 + SCAN_KINDS.index(kind), th=SCAN_TH.get(kind, 3.0))
    A = S.keyframe(T1_DEFAULT)
    entries = []
    for variant, val in items:
        u, v, z = _scan_geometry(kind, variant)
        if kind == "chi2_mono":
            p = S.point(A, u, v, z, 0); S.feature(A, u - 0.5, val, p, 10, octave=0)
        elif kind == "window_y":
            p = S.point(A, u, v, z, 0); S.feature(A, u, val, p, 10, octave=0)
        elif kind == "window_x":
            p = S.point(A, u, v, z, 0); S.feature(A, val, v, p, 10, octave=0)
        elif kind == "chi2_stereo":
            p = S.point(A, u, v, z, 0); S.feature(A, u, v, p, 10, octave=0, ur=val)
        else:
            X = tc.from_pixel(T1_DEFAULT, u, v, z); dist = np.linalg.norm(X - centre(T1_DEFAULT))
            if kind == "dist_min":
                p = S.point_at(A, X, 2, min_distance=val)
            elif kind == "dist_max":
                p = S.point_at(A, X, 0, max_distance=val, min_distance=dist / 8)
            else:
                n = _scan_normal(X); n[2] = val
                p = S.point_at(A, X, 2, normal=n)
            S.feature(A, u, v, p, 10, octave=0 if kind == "dist_max" else 2)
        entries.append(p)
    S.job(A, entries)
    return S.build("scan_" + kind)


def _scan_start(kind, variant):
    """(a value that is accepted, one that is rejected) of the sliding quantity, both positive, for the bisection."""
    small = 0.05 + 0.11 * variant
    u, v, z = _scan_geometry(kind, variant)
    if kind == "chi2_mono":
        return small + 0.4, small * 0.5                  # v - kp.y = 2.0 ... 2.4 + small / 2 (the bound: 2.396)
    if kind in ("window_x", "window_y"):
        return small + 0.5, small * 0.5                  # 1.5 px inside ... 2 + small / 2
    if kind == "chi2_stereo":
        return small + 2.8, small * 0.5                  # er = 0 ... 2.8 + small / 2 (the bound: 2.793)
    X = tc.from_pixel(T1_DEFAULT, u, v, z); dist = np.linalg.norm(X - centre(T1_DEFAULT))
    if kind == "dist_min":
        return dist / 0.9, dist / 0.7
    if kind == "dist_max":
        return dist / 1.1, dist / 1.3
    n = _scan_normal(X)
    assert n[2] > 0.2, "the viewing ray is mostly along z: the normal's z decides"
    return n[2] + 0.1, n[2] - 0.1


def scan_accepted(scene, contract="off"):
    """Per entry: fused (a hit)."""
    (best, hits, _), = cpu_run(scene, contract)[0]
    ok = np.zeros(len(best), bool); ok[hits["cand"]] = True
    return ok


def scan_scene(kind, steps=512):
    """`steps` entries in SCAN_WINDOWS windows: in each the sliding quantity takes consecutive f32 values centred on the bound `kind`
    names, for a geometry of its own.  The windows are placed by bisection with the ORACLE, all windows at once (one item each); the
    device never takes part."""
    W = SCAN_WINDOWS
    per = steps // W

    def accepted(vals):
        return scan_accepted(_scan_scene(kind, list(enumerate(vals))))

    start = [_scan_start(kind, v) for v in range(W)]
    lo = np.array([s[0] for s in start], F32); hi = np.array([s[1] for s in start], F32)
    assert np.all(lo > 0) and np.all(hi > 0), "the bisection walks the integer view of positive floats"
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


# ---------------------------------------------------------------- shapes and random scenes
def random_scene(seed, n_targets, n_points, n_features=300, mono_share=0.4, noise=0.6, lv=None, shared_list=True, state_share=0.3):
    """n_targets keyframes looking at one cloud of n_points map points; every target sees most of them as features (pixel noise, random
    octave around the predicted level, descriptor distance 0 - 70), stereo and mono mixed.  One candidate list shared by all jobs (the
    first loop of SearchInNeighbors) with a few -1 entries per job; random feature states."""
    rng = np.random.default_rng(4000 + 131 * seed + n_points + 7 * n_targets)
    lv = lv or Levels()
    S = SceneBuilder(100 + seed, lv=lv)
    T0 = pose(rodrigues(rng.normal(size=3) * 0.1), rng.normal(size=3))
    z = rng.uniform(4, 40, n_points); x = rng.uniform(-0.7, 0.7, n_points) * z; y = rng.uniform(-0.22, 0.22, n_points) * z
    Xw = to_world(T0, np.stack([x, y, z], 1))
    S.poses.append(T0)                                       # the points are made for the cloud's own pose
    for i in range(n_points):
        S.point_at(0, Xw[i], int(rng.integers(0, lv.nlevels)))
    S.poses.pop()
    for k in range(n_targets):
        T = tc.neighbour_pose(T0, rng.normal(size=3) * 0.5, rng.normal(size=3) * 0.03)
        K = S.keyframe(T)
        seen = rng.permutation(n_points)[:n_features]
        u, v, zc = project(T, Xw[seen])
        for j, i in enumerate(seen):
            if zc[j] <= 0.5:
                continue
            dist = np.linalg.norm(Xw[i] - centre(T))
            level = int(np.clip(np.ceil(np.log(float(S.points[i]["max_distance"]) / dist) / np.log(1.2)), 0, lv.nlevels - 1))
            octave = int(np.clip(level - int(rng.integers(0, 3)) + 1 - (rng.random() < 0.5), 0, lv.nlevels - 1))
            s = float(lv.scale[octave])
            stereo = rng.random() > mono_share
            S.feature(K, u[j] + rng.normal() * noise * s, v[j] + rng.normal() * noise * s, i, int(rng.integers(0, 71)), octave,
                      stereo_z=zc[j] * (1 + rng.normal() * 0.003) if stereo else None)
        entries = np.arange(n_points, dtype=np.int32) if shared_list else rng.permutation(n_points).astype(np.int32)[:max(1, n_points // 2)]
        entries = entries.copy(); entries[rng.random(len(entries)) < 0.05] = -1
        st = (rng.random(len(S.kfs[K].rows)) < state_share).astype(np.uint8) * rng.integers(1, 3, len(S.kfs[K].rows)).astype(np.uint8)
        S.job(K, entries, st)
    return S.build("random_%d_%d_%d" % (seed, n_targets, n_points))


def dense_window_scene(n_features, n_points=3, seed=0):
    """A window holding n_features features (more than one pass of the wave when > 64): all within 2 px of one projection, in several
    grid cells; the nearest descriptor sits late in the walk."""
    S = SceneBuilder(200 + seed + n_features)
    A = S.keyframe(T1_DEFAULT)
    rng = S.rng
    entries = []
    for q in range(n_points):
        wi, hi = GRID_COLS / 1241.0, GRID_ROWS / 376.0
        u, v = (12 + 9 * q + 0.5) / wi, (20 + 0.5) / hi        # a corner of four cells
        p = S.point(A, u, v, 10.0, 2)
        best_at = int(rng.integers(n_features // 2, n_features))
        for j in range(n_features):
            S.feature(A, u + rng.uniform(-2, 2), v + rng.uniform(-2, 2), p, 12 if j == best_at else int(rng.integers(13, 60)), octave=2)
        entries.append(p)
    S.job(A, entries)
    return S.build("dense_%d" % n_features)


def contention_scene(n_entries=40, seed=0):
    """A job whose hits all contend for one empty feature."""
    S = SceneBuilder(300 + seed)
    A = S.keyframe(T1_DEFAULT)
    fd = rand_desc(S.rng)
    S.kfs[A].add(400.0, 200.0, fd, 2)
    S.job(A, [S.point(A, 400.0 + 0.01 * j, 200.0, 10.0 + 0.1 * j, 2, desc=flipped(fd, int(S.rng.integers(0, 50)), S.rng)) for j in range(n_entries)])
    return S.build("contention")


def sized_jobs_scene(sizes=(0, 1, 63, 64, 65, 257), n_features=300, seed=0):
    """Jobs of the given entry counts over two keyframes that share slots between jobs."""
    sc = random_scene(30 + seed, 2, max(sizes), n_features)
    rng = np.random.default_rng(77 + seed)
    jobs = []
    for q, n in enumerate(sizes):
        k = q % 2
        e = rng.permutation(len(sc["points"]))[:n].astype(np.int32)
        jobs.append((k, e, sc["jobs"][k][2]))
    sc["jobs"] = jobs
    sc["name"] = "sized"
    return sc


def full_keyframe_scene(cap, seed=0):
    """A keyframe filled to the workspace's capacity."""
    S = SceneBuilder(400 + seed)
    A = S.keyframe(T1_DEFAULT)
    rng = S.rng
    entries = []
    for j in range(cap):
        u, v = rng.uniform(20, 1200), rng.uniform(10, 360)
        if j % 4 == 0:
            p = S.point(A, u, v, rng.uniform(5, 30), 2); entries.append(p)
            S.feature(A, u + rng.normal() * 0.5, v + rng.normal() * 0.5, p, int(rng.integers(0, 60)), octave=int(rng.integers(1, 3)))
        else:
            S.kfs[A].add(u, v, rand_desc(rng), int(rng.integers(0, 8)))
    S.job(A, entries)
    return S.build("full")


# ---------------------------------------------------------------- map-model scenes
def model_scene(seed, contention=True):
    """Keyframes and points with observations for the reformulation / snapshot tests.  Keyframe 0 is the target of job 0; keyframes 1
    and 2 hold the candidates' earlier observations (stereo and mono, so Observations() differ); keyframe 3 is a second target that
    sees the candidates which meet an occupant in keyframe 0.  -> scene + plan [(point, [(keyframe, feature)])], cand (the list every
    Fuse call gets), bad_feature (feature of keyframe 0, the bad point it holds), occupied [(candidate, occupant)]."""
    rng = np.random.default_rng(600 + seed)
    S = SceneBuilder(600 + seed)
    T0 = T1_DEFAULT
    K0 = S.keyframe(T0); K1 = S.keyframe(tc.neighbour_pose(T0, (0.6, 0.0, 0.1))); K2 = S.keyframe(tc.neighbour_pose(T0, (-0.5, 0.1, 0.0)))
    K3 = S.keyframe(tc.neighbour_pose(T0, (0.2, -0.3, 0.2)))
    plan, cand, occupied = [], [], []

    def obs_features(p, X, in_k1, in_k2):
        """One stereo observation in K1 (Observations() + 2) and / or one mono observation in K2 (+ 1)."""
        out = []
        for k, on, st in ((K1, in_k1, True), (K2, in_k2, False)):
            if on:
                u, v, zc = project(S.poses[k], X)
                out.append((k, S.feature(k, u[0], v[0], p, int(rng.integers(0, 20)), 2, stereo_z=zc[0] if st else None)))
        return out

    def candidate(u, v, z, d, in_k1=True, in_k2=False, feat=None, desc=None):
        """A candidate with observations in K1 / K2, aimed at K0's pixel (u, v); feat = an existing feature of K0 or None (a new one)."""
        X = tc.from_pixel(T0, u, v, z)
        p = S.point_at(K0, X, 2, desc=desc)
        f = S.feature(K0, u, v, p, d, 2, stereo_z=z) if feat is None else feat
        plan.append((p, obs_features(p, X, in_k1, in_k2)))
        cand.append(p)
        return p, f

    for j in range(4):                                  # plain adds
        candidate(150.0 + 90 * j, 80.0, 9.0 + j, 10 + 5 * j)
    # features of K0 (stereo: 2) that hold a point already: Observations() of (occupant, candidate) = (5, 2), (2, 3), (3, 3)
    for j, (occ, cnd) in enumerate((((True, True), (True, False)), ((False, False), (True, True)), ((False, True), (True, True)))):
        u, v, z = 150.0 + 90 * j, 160.0, 10.0 + j
        p, f = candidate(u, v, z, 12, in_k1=cnd[0], in_k2=cnd[1])
        X = tc.from_pixel(T0, u, v, z)
        q = S.point_at(K0, X, 2)
        plan.append((q, [(K0, f)] + obs_features(q, X, occ[0], occ[1])))
        occupied.append((p, q))
        u3, v3, z3 = project(S.poses[K3], X)
        S.feature(K3, u3[0], v3[0], p, 15, 2, stereo_z=z3[0])
    # a three-way contention on one empty mono feature, Observations() = 2, 3, 1
    if contention:
        fd = rand_desc(rng)
        f = S.kfs[K0].add(700.0, 120.0, fd, 2)
        for j, (a, b) in enumerate(((True, False), (True, True), (False, True))):
            candidate(700.0 + 0.2 * j, 120.0, 11.0 + 0.2 * j, None, in_k1=a, in_k2=b, feat=f, desc=flipped(fd, 8 + 6 * j, rng))
    # a feature that holds a bad point
    p, f = candidate(900.0, 200.0, 12.0, 9)
    bad = S.point_at(K0, tc.from_pixel(T0, 900.0, 200.0, 12.0), 2)
    sc = S.build("model_%d" % seed)
    sc.update(plan=plan, cand=np.array(cand, np.int32), bad_feature=(f, bad), occupied=occupied)
    return sc


def build_model(sc, contract="off"):
    """The model of a model_scene: every point with its planned observations, the bad point flagged bad, without observations but still
    in mvpMapPoints of keyframe 0 -> Model (point ids = indices into sc['points'])."""
    f, bad = sc["bad_feature"]
    M = Model(sc["kfs"], contract=contract)
    for i in range(len(sc["points"])):
        assert M.add_point(sc["points"][i], sc["pdesc"][i], bad=(i == bad)) == i
    for p, obs in sc["plan"]:
        for k, idx in obs:
            M.observe(p, k, idx)
    M.set_feature(0, f, bad)
    return M


# ---------------------------------------------------------------- the device side (tests marked gpu, tools)
class Workspace(tc.Workspace):
    """tc.Workspace plus the grid: upload() writes keyframes over slots, this runs sd_batch_assign_grid on them."""

    def upload_grid(self, kfs, cam=CAM):
        self.upload(kfs)
        self.b.assign_grid(len(kfs), cam)
        self.b.sync()


def device_run(ws, scene, cam=CAM, upload=True):
    """One sd_batch_fuse for all jobs of the scene -> [(best, hits, nfused)]."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    jobs = scene["jobs"]
    off = np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int32)
    ent = np.concatenate([j[1] for j in jobs] + [np.zeros(0, np.int32)]).astype(np.int32)
    d_ent = torch.from_numpy(ent).cuda() if len(ent) else None
    pts = np.ascontiguousarray(scene["points"], MP_DTYPE)
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda() if len(pts) else None
    d_desc = torch.from_numpy(np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1).copy()).cuda() if len(pts) else None
    d_state = None
    if any(j[2] is not None for j in jobs):
        st = np.zeros((len(jobs), ws.cap), np.uint8)
        for q, j in enumerate(jobs):
            if j[2] is not None:
                st[q, :len(j[2])] = j[2]
        d_state = torch.from_numpy(st).cuda()
    T = [scene["kfs"][j[0]]["Tcw"] for j in jobs]
    ws.b.fuse([j[0] for j in jobs], np.array(T, F32).reshape(len(jobs), 16) if jobs else np.zeros((0, 16), F32), off,
              d_ent.data_ptr() if d_ent is not None else None, d_pts.data_ptr() if d_pts is not None else None,
              d_desc.data_ptr() if d_desc is not None else None, cam, th=scene.get("th", 3.0),
              d_kf_state=d_state.data_ptr() if d_state is not None else None, n_points=len(pts))
    out = [ws.b.download_fuse(q) for q in range(len(jobs))]
    del d_ent, d_pts, d_desc, d_state
    return out


def assert_same(scene, got, want):
    for q, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], "%s job %d: nfused %d vs %d" % (scene["name"], q, g[2], w[2])
        assert g[0].tobytes() == w[0].tobytes(), "%s job %d: best differs at entries %r" % (scene["name"], q, np.nonzero((g[0] != w[0]).any(1))[0][:8])
        assert g[1].tobytes() == w[1].tobytes(), "%s job %d: hits differ" % (scene["name"], q)
    assert len(got) == len(want)
