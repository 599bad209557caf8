"""Shared by test_reloc_oracle.py, test_gpu_reloc.py and tools/fuzz_reloc.py: the CPU oracle of the relocalisation matcher
(tests/cpp/reloc_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory), a numpy restatement of it, and
seeded crafted scenes.

A scene is dict(name, kfs, points, pdesc, jobs): kfs = the image slots (frames and keyframes alike, as KeyFrameBuilder builds them),
points / pdesc = the sd_map_point table, jobs = [dict(frame=slot, kf=slot, Tcw, th, orb, kf_point (N1,), frame_point (N2,),
found (N1,) or None)].  A job is one ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist).
Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import fuse_cases as fc
import loop_cases as lc
import triangulate_cases as tc
from fuse_cases import MP_DTYPE, flipped, rand_desc
from triangulate_cases import CAM, F32, KP_DTYPE, KeyFrameBuilder, Levels, _p

ROOT = tc.ROOT
EXITS = ["", "null", "bad", "found", "out_u", "out_v", "dist_min", "dist_max", "window_empty", "no_free", "above_dist", "matched", "culled"]
X = {name: i for i, name in enumerate(EXITS) if name}
BRANCHES = ["null", "bad", "found", "out_u", "out_v", "dist_min", "dist_max", "window_empty", "no_free", "above_dist", "matched", "culled",
            "z_negative_searched", "nan_projection", "u_eq_minx", "u_eq_maxx", "v_eq_miny", "v_eq_maxy", "dist_eq_min", "dist_eq_max",
            "level_0", "level_top", "octave_below", "octave_above", "octave_lm1", "octave_l", "octave_lp1",
            "clip_left", "clip_right", "clip_top", "clip_bottom", "on_radius", "held_on_entry", "taken_by_earlier", "loser_second_choice",
            "tie_first_wins", "dist_eq_orb", "dist_orb_plus_1", "dist_256", "bin_wrap", "culled_had_blocked", "window_over_64", "no_features"]
TWINS = dict(none=0, tie_to_later_visit=1, lt_orbdist=2, z_positive=3, culled_freed_early=4, exclusive_max_bound=5, level_gate_of_sim3=6)
CASCADE_TWINS = dict(none=0, discard_after_second_optimisation=7, ge_30=8)
HISTO = 30
I4 = np.eye(4)

_oracles = {}


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast (to count the decisions that changes)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="reloc_oracle_")
        so = os.path.join(d, "libreloc_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []          # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "reloc_oracle.cpp"), os.path.join(ROOT, "tests", "cpp", "pose_oracle.cpp")])
        L = C.CDLL(so)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.sd_reloc_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_reloc_oracle_set_twin.argtypes = [i]
        L.sd_reloc_oracle_frame_new.restype = vp
        L.sd_reloc_oracle_frame_new.argtypes = [i, vp, vp, vp, i, vp]
        L.sd_reloc_oracle_frame_free.argtypes = [vp]
        L.sd_reloc_oracle_search.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f, i]
        L.sd_reloc_oracle_frame_set_stereo.argtypes = [vp, vp, vp]
        L.sd_reloc_oracle_refine.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        assert L.sd_reloc_oracle_branch_count() == len(BRANCHES)
        _oracles[contract] = L
    return _oracles[contract]


def cpu_search(scene, contract="off", twin="none", cam=CAM, lv=None):
    """Every job through the sequential oracle -> ([(frame_point (N2,), from_kf (N2,), exits (N1,), best (N1, 2), nmatches)], branches)."""
    L = oracle(contract)
    lv = lv or Levels()
    c = fc.cam_array(cam)
    hs = []
    for k in scene["kfs"]:
        kp = np.ascontiguousarray(k["kp"], KP_DTYPE); d = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1)
        hs.append(L.sd_reloc_oracle_frame_new(len(kp), _p(kp), _p(d), _p(c), lv.nlevels, _p(lv.scale)))
    L.sd_reloc_oracle_reset_branches(); L.sd_reloc_oracle_set_twin(TWINS[twin])
    p = np.ascontiguousarray(scene["points"], MP_DTYPE); d = np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1)
    out = []
    for j in scene["jobs"]:
        N1, N2 = len(scene["kfs"][j["kf"]]["kp"]), len(scene["kfs"][j["frame"]]["kp"])
        kfp = np.ascontiguousarray(j["kf_point"], np.int32); fp = np.full(max(N2, 1), -1, np.int32); fp[:N2] = j["frame_point"]
        assert len(kfp) == N1
        fnd = np.ascontiguousarray(j["found"], np.uint8) if j.get("found") is not None else None
        frm = np.full(max(N2, 1), -1, np.int32); ex = np.zeros(max(N1, 1), np.int32); best = np.zeros((max(N1, 1), 2), np.int32)
        T = np.ascontiguousarray(j["Tcw"], F32).reshape(16)
        nm = L.sd_reloc_oracle_search(hs[j["frame"]], hs[j["kf"]], _p(T), _p(kfp), _p(fnd), _p(p), _p(d), _p(fp), _p(frm), _p(ex), _p(best),
                                      float(j["th"]), int(j["orb"]))
        out.append((fp[:N2].copy(), frm[:N2].copy(), ex[:N1].copy(), best[:N1].copy(), nm))
    b = L.sd_reloc_oracle_branches()
    br = {name: int(b[i]) for i, name in enumerate(BRANCHES)}
    L.sd_reloc_oracle_set_twin(0)
    for h in hs:
        L.sd_reloc_oracle_frame_free(h)
    return out, br


# ---------------------------------------------------------------- numpy restatement
def _view_numpy(T, mp, cam):
    """-> exit name or (u, v, dist3D)"""
    Xw = mp["xw"].astype(F32)
    pc = [F32(F32(F32(T[i, 0] * Xw[0]) + F32(T[i, 1] * Xw[1])) + F32(T[i, 2] * Xw[2])) + T[i, 3] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F32(np.float64(1.0) / np.float64(pc[2]))
        u = F32(F32(cam["fx"] * pc[0]) * invz) + cam["cx"]; v = F32(F32(cam["fy"] * pc[1]) * invz) + cam["cy"]
    if u < cam["mnMinX"] or u > cam["mnMaxX"]:
        return "out_u"
    if v < cam["mnMinY"] or v > cam["mnMaxY"]:
        return "out_v"
    Ow = [F32(F32(F32(-T[0, i]) * T[0, 3]) + F32(F32(-T[1, i]) * T[1, 3])) + F32(F32(-T[2, i]) * T[2, 3]) for i in range(3)]
    PO = np.array([Xw[i] - Ow[i] for i in range(3)], F32).astype(np.float64)
    dist = F32(np.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]))
    if dist < F32(0.8) * mp["min_distance"]:
        return "dist_min"
    if dist > F32(1.2) * mp["max_distance"]:
        return "dist_max"
    return u, v, dist


def numpy_search(scene, cam=CAM, lv=None):
    lv = lv or Levels()
    out = []
    for j in scene["jobs"]:
        Fk, Kk = scene["kfs"][j["frame"]], scene["kfs"][j["kf"]]
        K = lc.NumpyKF(Fk, cam, lv)
        T = np.asarray(j["Tcw"], F32).reshape(4, 4)
        N1, N2 = len(Kk["kp"]), len(Fk["kp"])
        vp = np.asarray(j["frame_point"], np.int64).copy(); frm = np.full(N2, -1, np.int32)
        ex = np.zeros(N1, np.int32); best = np.tile(np.array([-1, 256], np.int32), (N1, 1)); bins = {}
        th, orb = F32(j["th"]), int(j["orb"])
        for i in range(N1):
            m = int(j["kf_point"][i])
            if m < 0:
                ex[i] = X["null"]; continue
            mp = scene["points"][m]
            if not mp["flags"] & 1:
                ex[i] = X["bad"]; continue
            if j.get("found") is not None and j["found"][i]:
                ex[i] = X["found"]; continue
            w = _view_numpy(T, mp, cam)
            if isinstance(w, str):
                ex[i] = X[w]; continue
            u, v, dist = w
            sel = np.zeros(0, np.int64)
            if not (np.isnan(u) or np.isnan(v)):
                ratio = F32(mp["max_distance"]) / dist
                level = int(np.ceil(F32(F32(np.log(np.float64(ratio))) / F32(np.log(np.float64(lv.scale[1]))))))
                level = min(max(level, 0), lv.nlevels - 1)
                sel = K.area(u, v, th * lv.scale[level])
                octv = Fk["kp"]["octave"][sel]
                sel = sel[(octv >= level - 1) & (octv <= level + 1)]
            if not len(sel):
                ex[i] = X["window_empty"]; continue
            sel = sel[vp[sel] == -1]
            d = lc._hamming_rows(scene["pdesc"][m], Fk["desc"][sel])
            q = int(np.argmin(d)) if len(sel) else -1
            if q < 0 or d[q] >= 256:
                ex[i] = X["no_free"]; continue
            best[i] = (sel[q], d[q])
            if d[q] > orb:
                ex[i] = X["above_dist"]; continue
            f = int(sel[q])
            vp[f] = m; frm[f] = i; ex[i] = X["matched"]
            rot = F32(Kk["kp"]["angle"][i]) - F32(Fk["kp"]["angle"][f])
            if rot < 0:
                rot = F32(rot + F32(360.0))
            b = int(np.floor(F32(rot * (F32(1.0) / F32(HISTO))) + F32(0.5)))
            bins[f] = 0 if (b == HISTO or b < 0 or b > HISTO) else b
        hist = np.bincount(np.array(list(bins.values()), np.int64), minlength=HISTO)
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
        for f, b in bins.items():
            if b not in (i1, i2, i3):
                ex[frm[f]] = X["culled"]; vp[f] = -1; frm[f] = -1
        out.append((vp.astype(np.int32), frm, ex, best, int((frm >= 0).sum())))
    return out


def assert_same(scene, got, want, what="device"):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        tag = "%s job %d (%s)" % (scene["name"], q, what)
        n1, n2 = len(w[2]), len(w[0])
        assert g[4] == w[4], "%s: nmatches %d vs %d" % (tag, g[4], w[4])
        assert g[2][:n1].tobytes() == w[2].tobytes(), "%s: exits differ at features %r: %r vs %r" % (
            tag, np.nonzero(g[2][:n1] != w[2])[0][:8], g[2][:n1][g[2][:n1] != w[2]][:8], w[2][g[2][:n1] != w[2]][:8])
        assert g[3][:n1].tobytes() == w[3].tobytes(), "%s: best differs at features %r" % (tag, np.nonzero((g[3][:n1] != w[3]).any(1))[0][:8])
        assert g[0][:n2].tobytes() == w[0].tobytes(), "%s: frame_point differs at %r" % (tag, np.nonzero(g[0][:n2] != w[0])[0][:8])
        assert g[1][:n2].tobytes() == w[1].tobytes(), "%s: from_kf differs at %r" % (tag, np.nonzero(g[1][:n2] != w[1])[0][:8])
        assert np.all(g[0][n2:] == -1) and np.all(g[1][n2:] == -1) and np.all(g[2][n1:] == X["null"]) and np.all(g[3][n1:] == (-1, 256)), tag + ": rows beyond the counts"


# ---------------------------------------------------------------- scene building
class Builder:
    """One frame (slot 0) and one keyframe (slot 1) under pose T.  pair() adds a map point seen at (u, v, z), the keyframe feature that
    holds it and (optionally) a frame feature near its projection; the keyframe's own key point positions never matter (only angles)."""

    def __init__(self, seed, T=I4, lv=None):
        self.rng = np.random.default_rng(12000 + seed)
        self.T, self.lv = np.asarray(T, np.float64), lv or Levels()
        self.F, self.K = KeyFrameBuilder(self.T), KeyFrameBuilder(I4)
        self.points, self.pdesc, self.kf_point, self.found, self.held = [], [], [], [], {}
        self.expect = {}

    def point(self, X, level=2, desc=None, bad=False, **kw):
        r = fc.point_record(self.T, np.asarray(X, np.float64), level, self.lv, **kw)
        if bad:
            r["flags"] = 0
        self.points.append(r); self.pdesc.append(rand_desc(self.rng) if desc is None else np.asarray(desc, np.uint8))
        return len(self.points) - 1

    def kf_feature(self, p=-1, angle=0.0, found=False):
        i = self.K.add(20.0 + 7.0 * (len(self.kf_point) % 160), 20.0 + 9.0 * (len(self.kf_point) // 160), rand_desc(self.rng), 0, angle)
        self.kf_point.append(p); self.found.append(1 if found else 0)
        return i

    def frame_feature(self, u, v, desc, octave=2, angle=0.0, held=None):
        f = self.F.add(u, v, desc, octave, angle)
        if held is not None:
            self.held[f] = held
        return f

    def pair(self, u, v, z=10.0, level=2, d=10, octave=None, off=(0.0, 0.0), kf_angle=0.0, frame_angle=0.0, feature=True, name=None, want=None, X=None, **kw):
        Xw = tc.from_pixel(self.T, u, v, z) if X is None else X
        p = self.point(Xw, level, **kw)
        i = self.kf_feature(p, kf_angle)
        f = self.frame_feature(u + off[0], v + off[1], flipped(self.pdesc[p], d, self.rng), level if octave is None else octave, frame_angle) if feature else -1
        if name:
            self.expect[name] = (i, want, f)
        return i, f, p

    def build(self, name, th=10.0, orb=100):
        pts = np.array(self.points, MP_DTYPE) if self.points else np.zeros(0, MP_DTYPE)
        Fk, Kk = self.F.build(), self.K.build()
        fp = np.full(len(Fk["kp"]), -1, np.int32)
        for f, m in self.held.items():
            fp[f] = m
        job = dict(frame=0, kf=1, Tcw=self.T.astype(F32), th=th, orb=orb, kf_point=np.array(self.kf_point, np.int32).reshape(-1), frame_point=fp,
                   found=np.array(self.found, np.uint8) if any(self.found) else None)
        return dict(name=name, kfs=[Fk, Kk], points=pts, pdesc=np.array(self.pdesc, np.uint8).reshape(len(pts), 32), jobs=[job], expect=self.expect)


def _anchors():
    i = 0
    while True:
        yield 70.0 + 90.0 * (i % 12), 45.0 + 70.0 * (i // 12)
        i += 1


def solve_factor(target, factor):
    """m (f32) with fl(factor * m) == target, or None."""
    m0 = F32(np.float64(target) / np.float64(factor))
    ms = (m0.view(np.int32) + np.arange(-8, 9, dtype=np.int32)).astype(np.int32).view(F32)
    ok = np.nonzero((F32(factor) * ms).astype(F32) == F32(target))[0]
    return ms[ok[len(ok) // 2]] if len(ok) else None


def dist_of(X):
    """dist3D of a point under the identity pose, as the matcher computes it."""
    P = np.asarray(X, F32).astype(np.float64)
    return F32(np.sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]))


def crafted_scene():
    """One job under the identity pose, th = 10, ORBdist = 100, every rule of the matcher at an anchor of its own (anchors are 90 x 70 px
    apart; the widest window, level 7, is below 36 px).  expect = {name: (keyframe feature, exit name, frame feature)}."""
    B = Builder(1)
    A = _anchors()
    rng = B.rng
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    # the bulk of the rotation histogram: plain matches at rot = 0 (bin 0)
    for q in range(12):
        u, v = next(A)
        B.pair(u, v, d=int(rng.integers(0, 40)), name="plain_%d" % q, want="matched")
    # the skips
    B.expect["null"] = (B.kf_feature(-1), "null", -1)
    u, v = next(A); B.pair(u, v, bad=True, name="bad", want="bad")
    u, v = next(A); i, f, p = B.pair(u, v, name="found", want="found"); B.found[i] = 1
    # no z > 0 test: a point behind the camera whose projection lies inside the image is searched
    u, v = next(A); B.pair(u, v, z=-10.0, name="z_negative", want="matched")
    # image bounds, both ends inside (v == mnMinY needs a camera of its own: v_min_scene)
    xm = float((F32(400.0) - cx) / fx); ym = float((F32(200.0) - cy) / fy)
    for name, target, horizontal, inside in (("u_eq_minx", CAM["mnMinX"], True, 5.0), ("u_eq_maxx", CAM["mnMaxX"], True, -11.0), ("v_eq_maxy", CAM["mnMaxY"], False, -6.0)):
        for beyond in (False, True):
            s = fc.solve_px(target, fx if horizontal else fy, cx if horizontal else cy)
            if beyond:
                s = np.nextafter(s, F32(-1e9) if inside > 0 else F32(1e9))
                while F32((fx if horizontal else fy) * s) + (cx if horizontal else cy) == target:
                    s = np.nextafter(s, F32(-1e9) if inside > 0 else F32(1e9))
            other = 120.0 if beyond else 60.0
            Xw = [float(s), float((F32(other) - cy) / fy), 1.0] if horizontal else [float((F32(other * 3) - cx) / fx), float(s), 1.0]
            pos = (float(target) + inside, other) if horizontal else (other * 3, float(target) + inside)
            p = B.point(Xw, 2); i = B.kf_feature(p)
            f = B.frame_feature(pos[0], pos[1], flipped(B.pdesc[p], 10, rng), 2)
            B.expect[name + ("_beyond" if beyond else "")] = (i, ("out_u" if horizontal else "out_v") if beyond else "matched", f)
    # distance bounds, both ends inside: min_distance / max_distance with fl(0.8f * min) == dist3D and fl(1.2f * max) == dist3D
    for name, factor in (("dist_eq_min", F32(0.8)), ("dist_eq_max", F32(1.2))):
        u, v = next(A); u2, v2 = next(A)
        for z in np.arange(10.0, 11.0, 0.01):
            Xw = tc.from_pixel(I4, u, v, z); dist = dist_of(Xw); m = solve_factor(dist, factor)
            if m is not None:
                break
        assert m is not None
        X2 = tc.from_pixel(I4, u2, v2, z); d2 = float(dist_of(X2))
        if factor < 1:        # the level comes from max_distance, left alone
            B.pair(u, v, X=Xw, min_distance=float(m), name=name, want="matched")
            B.pair(u2, v2, X=X2, min_distance=d2 / 0.8 * 1.001, name="dist_below_min", want="dist_min")
        else:                 # dist = 1.2 max: ratio = 1 / 1.2, level ceil(-1) clamps to 0
            B.pair(u, v, X=Xw, max_distance=float(m), min_distance=0.1, octave=0, name=name, want="matched")
            B.pair(u2, v2, X=X2, max_distance=d2 / 1.2 * 0.999, min_distance=0.1, octave=0, name="dist_above_max", want="dist_max")
    # the level gate: minLevel == -1 at level 0, maxLevel == nlevels at the top level, level - 2 ... level + 2 in between
    for level, octaves in ((0, ((0, True), (1, True), (2, False))), (7, ((5, False), (6, True), (7, True))), (3, ((1, False), (2, True), (3, True), (4, True), (5, False)))):
        for octv, hit in octaves:
            u, v = next(A)
            B.pair(u, v, level=level, octave=octv, name="level%d_octave%d" % (level, octv), want="matched" if hit else "window_empty")
    # the radius is strict: level 0, th = 10 -> r = 10 exactly; |dx| == 10 is outside, the float before it inside
    # (u = 4 so that u + dx is exact in f32)
    for name, dx, hit, (u, v) in (("on_radius", F32(10.0), False, (4.0, 200.0)), ("inside_radius", np.nextafter(F32(10.0), F32(0)), True, (4.0, 260.0))):
        xs = fc.solve_px(F32(u), fx, cx); ys = fc.solve_px(F32(v), fy, cy)
        p = B.point([float(xs), float(ys), 1.0], 0); i = B.kf_feature(p)
        f = B.frame_feature(float(F32(u) + dx), float(v), flipped(B.pdesc[p], 10, rng), 0)
        assert F32(F32(F32(u) + dx) - F32(u)) == dx
        B.expect[name] = (i, "matched" if hit else "window_empty", f)
    # no feature near the projection at all
    u, v = next(A); B.pair(u, v, feature=False, name="nothing_near", want="window_empty")
    # a member that holds a point on entry is no target: the farther free one is taken; alone, nothing is left
    u, v = next(A); i, f, p = B.pair(u, v, d=5); B.held[f] = p
    g = B.frame_feature(u + 2.0, v, flipped(B.pdesc[p], 30, rng), 2); B.expect["held_then_second"] = (i, "matched", g)
    u, v = next(A); i, f, p = B.pair(u, v, d=5, name="held_alone", want="no_free"); B.held[f] = p
    # acceptance: bestDist <= ORBdist
    u, v = next(A); B.pair(u, v, d=100, name="dist_eq_orb", want="matched")
    u, v = next(A); B.pair(u, v, d=101, name="dist_orb_plus_1", want="above_dist")
    # a lone member at distance 256 is never the best: bestIdx2 stays -1
    u, v = next(A); i, f, p = B.pair(u, v, name="dist_256", want="no_free"); B.F.desc[f] = np.bitwise_not(B.pdesc[p])
    # a tie: the first visit wins.  Same cell -> index order; two columns -> the left column first, whatever the index
    u, v = next(A); p = B.point(tc.from_pixel(I4, u, v, 10.0), 2); i = B.kf_feature(p); fd = flipped(B.pdesc[p], 20, rng)
    f1 = B.frame_feature(u + 1.0, v, fd, 2); B.frame_feature(u + 1.5, v, fd, 2); B.expect["tie_same_cell"] = (i, "matched", f1)
    wi = 64.0 / 1241.0
    ub = (round(u * wi) + 0.5) / wi                               # a column boundary
    p = B.point(tc.from_pixel(I4, ub, v + 30.0, 10.0), 2); i = B.kf_feature(p); fd = flipped(B.pdesc[p], 20, rng)
    fr = B.frame_feature(ub + 3.0, v + 30.0, fd, 2); fl = B.frame_feature(ub - 3.0, v + 30.0, fd, 2)
    assert fc.cell_of(ub + 3.0, v + 30.0)[0] == fc.cell_of(ub - 3.0, v + 30.0)[0] + 1
    B.expect["tie_left_column_first"] = (i, "matched", fl)
    # the greedy: an earlier keyframe feature takes the later one's best; the later takes its second choice / has none within ORBdist / none
    for name, second in (("second", 60), ("above", 120), ("none", None)):
        u, v = next(A); fd = rand_desc(rng); f = B.frame_feature(u, v, fd, 2)
        a, b = flipped(fd, 10, rng), flipped(fd, 20, rng)
        g = B.frame_feature(u + 2.0, v, flipped(b, second, rng), 2) if second else -1
        if second:
            assert tc.hamming(a, B.F.desc[g]) > 10
        X0 = tc.from_pixel(I4, u, v, 10.0)
        pa = B.point(X0, 2, desc=a); pb = B.point(X0, 2, desc=b)
        B.expect["greedy_%s_winner" % name] = (B.kf_feature(pa), "matched", f)
        B.expect["greedy_%s_loser" % name] = (B.kf_feature(pb), {"second": "matched", "above": "above_dist", "none": "no_free"}[name], g)
    # rotation: rot = 100 degrees (bin 3) is removed after the loop, and it blocked a later feature while the loop ran
    u, v = next(A); fd = rand_desc(rng); f = B.frame_feature(u, v, fd, 2, angle=0.0)
    a, b = flipped(fd, 10, rng), flipped(fd, 20, rng)
    g = B.frame_feature(u + 2.0, v, flipped(b, 60, rng), 2)
    X0 = tc.from_pixel(I4, u, v, 10.0)
    pa = B.point(X0, 2, desc=a); pb = B.point(X0, 2, desc=b)
    B.expect["culled_blocker"] = (B.kf_feature(pa, angle=100.0), "culled", f)
    B.expect["blocked_by_culled"] = (B.kf_feature(pb), "matched", g)
    # rot < 0 wraps by 360 (355 degrees: bin 12, removed); a difference of 899 degrees reaches bin 30, which is bin 0 (kept)
    u, v = next(A); B.pair(u, v, kf_angle=0.0, frame_angle=5.0, name="rot_negative", want="culled")
    u, v = next(A); B.pair(u, v, kf_angle=899.0, frame_angle=0.0, name="bin_wrap", want="matched")
    sc = B.build("crafted")
    return sc


def check_expect(scene, results):
    fp, frm, ex, best, nm = results[0]
    for name, (i, want, f) in scene["expect"].items():
        assert EXITS[ex[i]] == want, "%s: exit %s, meant %s" % (name, EXITS[ex[i]], want)
        if want == "matched":
            assert frm[f] == i and best[i][0] == f, "%s: feature %d meant to take %d, took %d" % (name, i, f, best[i][0])
        if want == "culled":
            assert frm[f] == -1 and fp[f] == -1 and best[i][0] == f, name


CAM_VMIN = lc.CAM_VMIN


def v_min_scene():
    """v exactly ON mnMinY (inside) and the next f32 ordinate beyond it (outside), under CAM_VMIN and the identity pose."""
    B = Builder(2)
    cam = CAM_VMIN
    x_mid = float((F32(400.0) - cam["cx"]) / cam["fx"])
    on = F32(-0.25); beyond = np.nextafter(on, F32(-1))
    assert F32(cam["fy"] * on) + cam["cy"] == cam["mnMinY"] and F32(cam["fy"] * beyond) + cam["cy"] < cam["mnMinY"]
    for name, y, dx, want in (("v_eq_miny", on, 0.0, "matched"), ("v_below_miny", beyond, 40.0, "out_v")):
        p = B.point([x_mid + dx / float(cam["fx"]), float(y), 1.0], 2); i = B.kf_feature(p)
        f = B.frame_feature(400.0 + dx, 1.0, flipped(B.pdesc[p], 10, B.rng), 2)
        B.expect[name] = (i, want, f)
    return B.build("v_min")


def nan_scene():
    """zc == 0 with xc == 0: invzc = inf, u = NaN passes both image tests; GetFeaturesInArea finds nothing.  With xc != 0 u is infinite."""
    B = Builder(3)
    for name, Xw, want in (("nan", [0.0, 0.0, 0.0], "window_empty"), ("inf", [1.0, 0.0, 0.0], "out_u")):
        r = np.zeros((), MP_DTYPE); r["xw"] = Xw; r["normal"] = (0, 0, 1); r["min_distance"] = 0.0; r["max_distance"] = 5.0; r["flags"] = 1
        B.points.append(r); B.pdesc.append(rand_desc(B.rng)); B.expect[name] = (B.kf_feature(len(B.points) - 1), want, -1)
    B.frame_feature(float(CAM["cx"]), float(CAM["cy"]), rand_desc(B.rng), 0)
    return B.build("nan")


def sized_scene(n_kf, n_frame=None, seed=0):
    """n_kf keyframe features, each with a point of its own on a grid of anchors and one frame feature near it (n_frame = 0: a frame
    without features)."""
    B = Builder(100 + n_kf + seed)
    for q in range(n_kf):
        u, v = 30.0 + 40.0 * (q % 29), 20.0 + 40.0 * (q // 29)
        B.pair(u, v, d=int(B.rng.integers(0, 60)), feature=n_frame != 0, off=(float(B.rng.uniform(-2, 2)), float(B.rng.uniform(-2, 2))))
    return B.build("sized_%d_%s" % (n_kf, n_frame))


def dense_window_scene(n_members, n_takers, seed=0):
    """n_members free frame features within ORBdist of n_takers identical points in one window: taker k finds its k - 1 nearest taken.
    With more members than SD_PROJ_K = 64 kept keys, taker 65 needs the 65th key."""
    B = Builder(200 + n_members + seed)
    d0 = rand_desc(B.rng)
    for j in range(n_members):
        B.frame_feature(400.0 + 0.05 * j, 200.0, flipped(d0, j % 40, B.rng), 2)
    X0 = tc.from_pixel(I4, 401.0, 200.0, 10.0)
    for k in range(n_takers):
        B.kf_feature(B.point(X0, 2, desc=d0))
    return B.build("dense_%d_%d" % (n_members, n_takers), th=3.0, orb=64)


def chain_scene(n=65):
    """n keyframe features, each displaced by the one before it: feature i prefers frame feature i - 1 (taken by feature i - 1) and
    takes frame feature i.  A round of the device's replay commits one of them; the chain crosses the chunk of 64."""
    B = Builder(300 + n)
    fd = [rand_desc(B.rng)]
    for _ in range(n):
        fd.append(flipped(fd[-1], 100, B.rng))                    # neighbours 100 bits apart: feature i is 40 from fd[i - 1], 60 from fd[i]
    v = 200.0
    for j in range(n + 1):
        B.frame_feature(100.0 + 6.0 * j, v, fd[j], 2)
    want = []
    for i in range(n):
        desc = flipped(fd[0], 10, B.rng) if i == 0 else lc._toward(fd[i - 1], fd[i], 40, B.rng)
        p = B.point(tc.from_pixel(I4, 100.0 + 6.0 * i - (3.0 if i else 0.0), v, 10.0), 2, desc=desc)
        B.kf_feature(p); want.append(i)
    sc = B.build("chain_%d" % n)
    sc["want_chain"] = want
    return sc


def random_scene(seed, n_kf=260, n_frame=300, n_jobs=3, T=None):
    """(n_frame points, each with a frame feature and three in ten with a second one.)  A frame (slot 0) and n_jobs keyframes (slots 1 ..) over one point table: most keyframe features hold a point that projects into the
    frame with a feature nearby (noise of a few pixels, 0 .. 120 bits apart, octave around the predicted level), some frame features
    hold a point on entry, some points are bad or already found, angles come from a few clusters so that the histogram removes some.
    Jobs alternate (th, ORBdist) = (10, 100) and (3, 64), the two settings of Relocalization."""
    rng = np.random.default_rng(13000 + seed)
    T = tc.T1_DEFAULT if T is None else T
    lv = Levels()
    F = KeyFrameBuilder(T)
    pts, pdesc = [], []
    for q in range(n_frame):
        u, v = rng.uniform(1, 1229), rng.uniform(1, 371)
        z = rng.uniform(4, 40) * (-1 if rng.random() < 0.03 else 1)
        level = int(rng.integers(0, lv.nlevels))
        Xw = tc.from_pixel(np.asarray(T, np.float64), u, v, z)
        pts.append(fc.point_record(np.asarray(T, np.float64), Xw, level, lv)); pdesc.append(rand_desc(rng))
        r = rng.random()
        if r < 0.04:                                              # outside the scale pyramid, on either side
            pts[-1]["min_distance"] = pts[-1]["max_distance"]
        elif r < 0.08:
            pts[-1]["max_distance"] *= F32(0.6); pts[-1]["min_distance"] *= F32(0.6)
        if rng.random() < 0.05:
            pts[-1]["flags"] = 0
        octv = int(np.clip(level + rng.integers(-2, 3), 0, lv.nlevels - 1))
        F.add(u + rng.normal(0, 2.0), v + rng.normal(0, 2.0), flipped(pdesc[-1], int(rng.integers(0, 121)), rng), octv, float(rng.choice([0.0, 3.0, 40.0, 200.0])))
        if rng.random() < 0.3:                                    # a second choice for whoever loses the first
            F.add(u + rng.normal(0, 2.0), v + rng.normal(0, 2.0), flipped(pdesc[-1], int(rng.integers(20, 91)), rng), octv, float(rng.choice([0.0, 3.0])))
    Fk = F.build()
    n_points, n_frame = n_frame, len(Fk["kp"])
    kfs, jobs = [Fk], []
    for j in range(n_jobs):
        K = KeyFrameBuilder(I4)
        kfp = np.full(n_kf, -1, np.int32)
        for i in range(n_kf):
            K.add(rng.uniform(5, 1225), rng.uniform(5, 368), rand_desc(rng), 0, float(rng.choice([0.0, 5.0, 45.0, 250.0], p=[0.6, 0.2, 0.15, 0.05])))
            if rng.random() < 0.8:
                kfp[i] = int(rng.integers(0, n_points))           # with repetition: two features may carry one point
        fp = np.full(n_frame, -1, np.int32)
        heldi = rng.choice(n_frame, n_frame // 6, replace=False)
        fp[heldi] = rng.integers(0, n_points, len(heldi))
        found = (rng.random(n_kf) < 0.1).astype(np.uint8)
        Tj = tc.pose(tc.rodrigues(rng.normal(0, 0.004, 3)), rng.normal(0, 0.05, 3)) @ np.asarray(T, np.float64)      # border points leave the image
        kfs.append(K.build())
        jobs.append(dict(frame=0, kf=1 + j, Tcw=Tj.astype(F32), th=10.0 if j % 2 == 0 else 3.0, orb=100 if j % 2 == 0 else 64, kf_point=kfp, frame_point=fp, found=found))
    return dict(name="random_%d" % seed, kfs=kfs, points=np.array(pts, MP_DTYPE), pdesc=np.array(pdesc, np.uint8).reshape(-1, 32), jobs=jobs, expect={})


# ---------------------------------------------------------------- 1-ulp scans
SCAN_KINDS = ("u_min", "u_max", "v_min", "v_max", "dist_min", "dist_max", "radius", "level_1", "level_4", "level_7")
SCAN_STEPS, SCAN_VARIANTS = 512, 4


def scan_scene(kind):
    """512 keyframe features in one job, 4 geometries x 128 consecutive f32 values of the quantity that `kind` slides across its bound,
    centred on the crossing the ORACLE finds.  All items of a geometry look at one frame feature, so only the first that reaches it is
    matched; the decision under test is the exit (out_u / dist_min / window_empty / ... against matched or no_free).
    u_*, v_*: the abscissa / ordinate of a point at depth 1 (v_min under CAM_VMIN).  dist_*: min_distance / max_distance of a fixed point.
    radius: the abscissa of a point whose projection approaches a feature 10 px away at level 0 (th 10).  level_k: max_distance across
    the step of PredictScale from k - 1 to k, the feature's octave k + 1 being inside only at level k (at the top level: octave k - 2, inside
    only at level k - 1)."""
    per = SCAN_STEPS // SCAN_VARIANTS
    cam = CAM_VMIN if kind == "v_min" else CAM
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    lv = Levels()

    def build(values):
        """values[variant] = the sliding f32 values of that geometry"""
        B = Builder(400 + SCAN_KINDS.index(kind))
        for var, vals in enumerate(values):
            if kind in ("u_min", "u_max", "v_min", "v_max"):
                horizontal = kind[0] == "u"
                target = {"u_min": cam["mnMinX"], "u_max": cam["mnMaxX"], "v_min": cam["mnMinY"], "v_max": cam["mnMaxY"]}[kind]
                inside = 5.0 if kind.endswith("min") else (-11.0 if horizontal else -6.0)
                other = 60.0 + 70.0 * var
                pos = (float(target) + inside, other) if horizontal else (other * 3, float(target) + inside)
                d0 = rand_desc(B.rng); B.frame_feature(pos[0], pos[1], d0, 2)
                for s in vals:
                    z = 1.0 + 0.37 * var                          # depth 1 makes invzc exact; the other geometries round it
                    Xw = [float(s), float((F32(other) - cy) / fy) * z, z] if horizontal else [float((F32(other * 3) - cx) / fx) * z, float(s), z]
                    B.kf_feature(B.point(Xw, 2, desc=d0))
            elif kind in ("dist_min", "dist_max"):
                u, v = 100.0 + 250.0 * var, 100.0 + 40.0 * var
                Xw = tc.from_pixel(I4, u, v, 9.0 + var); d0 = rand_desc(B.rng)
                B.frame_feature(u, v, d0, 0 if kind == "dist_max" else 2)
                for s in vals:
                    kw = dict(min_distance=float(s)) if kind == "dist_min" else dict(max_distance=float(s), min_distance=0.1)
                    B.kf_feature(B.point(Xw, 2, desc=d0, **kw))
            elif kind == "radius":
                u, v = 150.0 + 250.0 * var, 90.0 + 60.0 * var
                d0 = rand_desc(B.rng); B.frame_feature(u + 10.0, v, d0, 0)
                for s in vals:
                    B.kf_feature(B.point([float(s), float((F32(v) - cy) / fy), 1.0], 0, desc=d0))
            else:
                k = int(kind[-1])
                u, v = 150.0 + 250.0 * var, 90.0 + 60.0 * var
                Xw = tc.from_pixel(I4, u, v, 9.0 + var); d0 = rand_desc(B.rng)
                B.frame_feature(u, v, d0, k + 1 if k < lv.nlevels - 1 else k - 2)
                for s in vals:
                    B.kf_feature(B.point(Xw, 2, desc=d0, max_distance=float(s), min_distance=0.01))
        return B.build("scan_" + kind)

    def start(var):
        """(a value on the `reached` side, a value on the other side)"""
        if kind in ("u_min", "u_max", "v_min", "v_max"):
            f, c = (fx, cx) if kind[0] == "u" else (fy, cy)
            t = {"u_min": cam["mnMinX"], "u_max": cam["mnMaxX"], "v_min": cam["mnMinY"], "v_max": cam["mnMaxY"]}[kind]
            z = 1.0 + 0.37 * var
            x = float((np.float64(t) - np.float64(c)) / np.float64(f)) * z; step = 2.0 / float(f) * z
            return (x + step, x - step) if kind.endswith("min") else (x - step, x + step)
        if kind in ("dist_min", "dist_max"):
            dist = float(dist_of(tc.from_pixel(I4, 100.0 + 250.0 * var, 100.0 + 40.0 * var, 9.0 + var)))
            return (dist / 0.8 * 0.999, dist / 0.8 * 1.001) if kind == "dist_min" else (dist / 1.2 * 1.001, dist / 1.2 * 0.999)
        if kind == "radius":
            x = float((np.float64(150.0 + 250.0 * var) - np.float64(cx)) / np.float64(fx)); step = 1.0 / float(fx)
            return (x + step, x - step)
        k = int(kind[-1])
        dist = float(dist_of(tc.from_pixel(I4, 150.0 + 250.0 * var, 90.0 + 60.0 * var, 9.0 + var)))
        edge = dist * float(lv.scale_factor) ** (k - 1)          # ceil(log(max / dist) / log 1.2) steps from k - 1 to k just above it
        return (edge * 1.001, edge * 0.999) if k < lv.nlevels - 1 else (edge * 0.999, edge * 1.001)

    def reached(values):
        """per item: the matcher got as far as the feature (matched / no_free) instead of the exit under test"""
        (fp, frm, ex, best, nm), = cpu_search(build(values), cam=cam)[0]
        return np.isin(ex, (X["matched"], X["no_free"])).reshape(len(values), -1)

    st = [start(v) for v in range(SCAN_VARIANTS)]
    lo = np.array([s[0] for s in st], F32); hi = np.array([s[1] for s in st], F32)
    assert np.all((lo < 0) == (hi < 0)), "the bisection walks the integer view of floats of one sign"
    r_lo, r_hi = reached([[x] for x in lo]), reached([[x] for x in hi])
    assert r_lo.all() and not r_hi.any(), (kind, r_lo.ravel(), r_hi.ravel())
    li, hj = lo.view(np.int32).astype(np.int64), hi.view(np.int32).astype(np.int64)
    while np.any(np.abs(hj - li) > 1):
        mid = (li + hj) // 2
        ok = reached([[x] for x in mid.astype(np.int32).view(F32)])[:, 0]
        li, hj = np.where(ok, mid, li), np.where(ok, hj, mid)
    values = []
    for v in range(SCAN_VARIANTS):
        first = min(li[v], hj[v]) - per // 2 + 1
        values.append((first + np.arange(per)).astype(np.int32).view(F32))
    sc = build(values)
    sc["cam"] = cam
    return sc


def scan_reached(scene, contract="off"):
    (fp, frm, ex, best, nm), = cpu_search(scene, contract, cam=scene["cam"])[0]
    return np.isin(ex, (X["matched"], X["no_free"]))


# ---------------------------------------------------------------- the device side (tests marked gpu, tools)
Workspace = fc.Workspace


def device_search(ws, scene, cam=CAM, upload=True, jobs=None):
    """One sd_batch_search_by_projection_reloc for the jobs of the scene -> [(frame_point (cap,), from_kf (cap,), exits (cap,), best (cap, 2), nmatches)]."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    jobs = scene["jobs"] if jobs is None else jobs
    n = len(jobs)
    kfp = np.full((max(n, 1), ws.cap), -1, np.int32); fp = np.full((max(n, 1), ws.cap), -1, np.int32); fnd = np.zeros((max(n, 1), ws.cap), np.uint8)
    for q, j in enumerate(jobs):
        kfp[q, :len(j["kf_point"])] = j["kf_point"]; fp[q, :len(j["frame_point"])] = j["frame_point"]
        if j.get("found") is not None:
            fnd[q, :len(j["found"])] = j["found"]
    pts = np.ascontiguousarray(scene["points"], MP_DTYPE)
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda() if len(pts) else None
    d_desc = torch.from_numpy(np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1).copy()).cuda() if len(pts) else None
    d_kfp, d_fp = torch.from_numpy(kfp).cuda(), torch.from_numpy(fp).cuda()
    d_fnd = torch.from_numpy(fnd).cuda() if any(j.get("found") is not None for j in jobs) else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    T = np.array([np.asarray(j["Tcw"], F32).reshape(16) for j in jobs], F32).reshape(n, 16)
    ws.b.search_by_projection_reloc([j["frame"] for j in jobs], [j["kf"] for j in jobs], T, np.array([j["th"] for j in jobs], F32),
                                    np.array([j["orb"] for j in jobs], np.int32), d_kfp.data_ptr(), d_fp.data_ptr(), ptr(d_pts), ptr(d_desc), cam,
                                    d_found=ptr(d_fnd), n_points=len(pts))
    out = [ws.b.download_reloc_matches(q) for q in range(n)]
    del d_pts, d_desc, d_kfp, d_fp, d_fnd
    return out


# ---------------------------------------------------------------- the cascade of Tracking::Relocalization (Tracking.cc:2292-2358)
RESULT_DTYPE = np.dtype([("stage_reached", "<i4"), ("matched", "<i4"), ("n_good", "<i4", (3,)), ("n_additional", "<i4", (2,)),
                         ("Tcw_stage", "<f4", (3, 4, 4)), ("Tcw", "<f4", (4, 4))])      # sd_reloc_result
POSE_TOL = 1e-5           # pose_cases.pose_close: the bar the device's PoseOptimization is held to


def cpu_refine(scene, twin="none", perturb=None, cam=CAM, lv=None):
    """Every job through the sequential cascade -> [(result (RESULT_DTYPE scalar), frame_point (N2,), outlier (N2,))].
    perturb: (n_jobs, 3, 16) f32 added to the pose after each optimisation."""
    L = oracle()
    lv = lv or Levels()
    c = fc.cam_array(cam); iv = fc.inv_sigma2(lv)
    hs = []
    for k in scene["kfs"]:
        kp = np.ascontiguousarray(k["kp"], KP_DTYPE); d = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1); ur = np.ascontiguousarray(k["ur"], F32)
        h = L.sd_reloc_oracle_frame_new(len(kp), _p(kp), _p(d), _p(c), lv.nlevels, _p(lv.scale))
        L.sd_reloc_oracle_frame_set_stereo(h, _p(ur), _p(iv))
        hs.append(h)
    L.sd_reloc_oracle_set_twin(CASCADE_TWINS[twin])
    p = np.ascontiguousarray(scene["points"], MP_DTYPE); d = np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1)
    out = []
    for q, j in enumerate(scene["jobs"]):
        N2 = len(scene["kfs"][j["frame"]]["kp"])
        kfp = np.ascontiguousarray(j["kf_point"], np.int32); fp = np.full(max(N2, 1), -1, np.int32); fp[:N2] = j["frame_point"]
        o = np.zeros(max(N2, 1), np.uint8); res = np.zeros(1, RESULT_DTYPE)
        T = np.ascontiguousarray(j["Tcw"], F32).reshape(16)
        pt = np.ascontiguousarray(perturb[q], F32).reshape(48) if perturb is not None else None
        L.sd_reloc_oracle_refine(hs[j["frame"]], hs[j["kf"]], _p(T), _p(kfp), _p(p), _p(d), _p(fp), _p(o), _p(res), _p(pt))
        out.append((res[0].copy(), fp[:N2].copy(), o[:N2].copy()))
    L.sd_reloc_oracle_set_twin(0)
    for h in hs:
        L.sd_reloc_oracle_frame_free(h)
    return out


def decisions(r):
    """What of a cascade result must not depend on the last bits of a pose."""
    res, fp, o = r
    return (int(res["stage_reached"]), int(res["matched"]), tuple(int(x) for x in res["n_good"]), tuple(int(x) for x in res["n_additional"]),
            fp.tobytes(), o.tobytes())


def pose_perturbation(rng, T):
    """A (3, 16) perturbation of the size pose_close tolerates: POSE_TOL on the rotation, POSE_TOL * max(1, |t|) on the translation."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    d = np.zeros((3, 4, 4))
    d[:, :3, :3] = rng.choice([-1.0, 1.0], (3, 3, 3)) * POSE_TOL
    d[:, :3, 3] = rng.choice([-1.0, 1.0], (3, 3)) * POSE_TOL * max(1.0, float(np.linalg.norm(T[:3, 3])))
    return d.reshape(3, 16).astype(F32)


# name -> (BoW inliers that fit, BoW inliers that do not, then what the first search adds: good / 8 px off at rotation 0, groups at 45 and
# 250 degrees, the group at 100 degrees that the first search's histogram removes and the second search finds, how many of that group lie
# 4 px off) and what must come out: (stage_reached, matched, n_good, n_additional).  Every count sits ON a gate of lines 2313 - 2354.
CASCADE_CASES = {
    "2313_ngood_9":    ((9, 3, 5, 0, 0, 0, 0, 0),     (1, 0, (9, -1, -1), (-1, -1))),
    "2313_ngood_10":   ((10, 3, 5, 0, 0, 0, 0, 0),    (2, 0, (10, -1, -1), (5, -1))),
    "2321_ngood_49":   ((49, 2, 1, 0, 0, 0, 0, 0),    (3, 1, (49, 50, -1), (1, -1))),
    "2321_ngood_50":   ((50, 2, 4, 0, 0, 0, 0, 0),    (1, 1, (50, -1, -1), (-1, -1))),
    "2325_sum_49":     ((20, 2, 29, 0, 0, 0, 0, 0),   (2, 0, (20, -1, -1), (29, -1))),
    "2325_sum_50":     ((20, 2, 30, 0, 0, 0, 0, 0),   (3, 1, (20, 50, -1), (30, -1))),
    "2331_ngood_30":   ((12, 2, 18, 20, 0, 0, 0, 0),  (3, 0, (12, 30, -1), (38, -1))),
    "2331_ngood_31":   ((13, 2, 18, 19, 0, 0, 0, 0),  (4, 0, (13, 31, -1), (37, 0))),
    "2331_ngood_49":   ((20, 2, 29, 1, 0, 0, 0, 0),   (4, 0, (20, 49, -1), (30, 0))),
    "2340_sum_49":     ((15, 2, 14, 5, 8, 8, 4, 0),   (4, 0, (15, 45, -1), (35, 4))),
    "2340_sum_50":     ((15, 2, 14, 5, 8, 8, 5, 0),   (5, 1, (15, 45, 50), (35, 5))),
    "2354_ngood_49":   ((15, 2, 14, 5, 8, 8, 5, 1),   (5, 0, (15, 45, 49), (35, 5))),
}


def cascade_scene(names=None, seed=0):
    """One job per named case (all, in order, by default): slots 2q (frame) and 2q + 1 (keyframe) of case q.  The true pose is the
    identity; Tcw of a job is that pose turned by 2 mrad and moved by a centimetre, as a PnP estimate would be.  Features that fit lie
    on the exact projection, those that do not 30 px (BoW) / 8 px (first search) / 4 px (second search) away: the residuals are either
    below 1e-3 px or many times the chi-square bound, and every window holds its feature with a pixel to spare, so no decision hangs on
    the last bits of a pose (test_reloc_oracle.py checks it)."""
    names = list(CASCADE_CASES) if names is None else list(names)
    kfs, jobs, pts, pdesc, want = [], [], [], [], []
    for q, name in enumerate(names):
        (n_in, n_bow_bad, good0, bad0, a, b_, g, g_bad), expect = CASCADE_CASES[name]
        B = Builder(500 + 37 * list(CASCADE_CASES).index(name) + seed)
        rng = B.rng
        k = [0]

        def anchor():
            i = k[0]; k[0] += 1
            return 40.0 + 60.0 * (i % 20), 25.0 + 45.0 * (i // 20)

        def add(off, kf_angle, held):
            u, v = anchor(); z = float(rng.uniform(6, 20))
            p = B.point(tc.from_pixel(I4, u, v, z), 2); i = B.kf_feature(p, kf_angle)
            f = B.F.add(u + off[0], v + off[1], flipped(B.pdesc[p], int(rng.integers(0, 40)), rng), 2, 0.0, stereo_z=z if (k[0] % 3 == 0 and off == (0.0, 0.0)) else None)
            if held:
                B.held[f] = p

        dirs = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
        for n in range(n_in):
            add((0.0, 0.0), 0.0, True)
        for n in range(n_bow_bad):
            add((30.0 * dirs[n % 4][0], 30.0 * dirs[n % 4][1]), 0.0, True)
        for n in range(good0):
            add((0.0, 0.0), 0.0, False)
        for n in range(bad0):
            add((8.0 * dirs[n % 4][0], 8.0 * dirs[n % 4][1]), 0.0, False)
        for n in range(a):
            add((0.0, 0.0), 45.0, False)
        for n in range(b_):
            add((0.0, 0.0), 250.0, False)
        for n in range(g):
            add((4.0, 0.0) if n < g_bad else (0.0, 0.0), 100.0, False)
        sc = B.build(name)
        job = sc["jobs"][0]
        job["frame"], job["kf"] = 2 * q, 2 * q + 1
        job["Tcw"] = (tc.pose(tc.rodrigues([0.002, -0.001, 0.0015]), [0.01, -0.006, 0.008])).astype(F32)
        job["kf_point"] = np.where(job["kf_point"] >= 0, job["kf_point"] + len(pts), -1).astype(np.int32)
        job["frame_point"] = np.where(job["frame_point"] >= 0, job["frame_point"] + len(pts), -1).astype(np.int32)
        job["found"] = None
        kfs += sc["kfs"]; jobs.append(job); pts += list(sc["points"]); pdesc += list(sc["pdesc"]); want.append(expect)
    return dict(name="cascade", kfs=kfs, jobs=jobs, points=np.array(pts, MP_DTYPE), pdesc=np.array(pdesc, np.uint8).reshape(-1, 32), names=names, want=want)


def random_cascade_scene(seed, n_jobs=3):
    """Cascades as a tracker would meet them: per job a frame of 40 .. 140 true correspondences of which a share is known on entry (the BoW
    inliers), a tenth of those wrong, pixel noise of 0.3 px.  The counts stay away from 10 / 30 / 50 by construction of nothing: the fuzz
    tool counts the draws whose decisions hang on the pose."""
    rng = np.random.default_rng(14000 + seed)
    kfs, jobs, pts, pdesc = [], [], [], []
    for q in range(n_jobs):
        B = Builder(14000 + 10 * seed + q)
        n = int(rng.integers(40, 141)); known = float(rng.uniform(0.1, 0.7))
        for i in range(n):
            u, v = 30.0 + 48.0 * (i % 25), 20.0 + 50.0 * (i // 25); z = float(rng.uniform(5, 30))
            p = B.point(tc.from_pixel(I4, u, v, z), 2); B.kf_feature(p, float(rng.choice([0.0, 0.0, 0.0, 20.0, 200.0])))
            held = rng.random() < known
            off = rng.normal(0, 0.3, 2) + (rng.choice([-25.0, 25.0], 2) if held and rng.random() < 0.1 else 0.0)
            f = B.F.add(u + off[0], v + off[1], flipped(B.pdesc[p], int(rng.integers(0, 90)), rng), int(rng.integers(1, 4)), 0.0, stereo_z=z if rng.random() < 0.3 else None)
            if held:
                B.held[f] = p
        sc = B.build("random_cascade_%d_%d" % (seed, q))
        job = sc["jobs"][0]
        job["frame"], job["kf"] = 2 * q, 2 * q + 1
        job["Tcw"] = (tc.pose(tc.rodrigues(rng.normal(0, 0.002, 3)), rng.normal(0, 0.01, 3))).astype(F32)
        job["kf_point"] = np.where(job["kf_point"] >= 0, job["kf_point"] + len(pts), -1).astype(np.int32)
        job["frame_point"] = np.where(job["frame_point"] >= 0, job["frame_point"] + len(pts), -1).astype(np.int32)
        job["found"] = None
        kfs += sc["kfs"]; jobs.append(job); pts += list(sc["points"]); pdesc += list(sc["pdesc"])
    return dict(name="random_cascade_%d" % seed, kfs=kfs, jobs=jobs, points=np.array(pts, MP_DTYPE), pdesc=np.array(pdesc, np.uint8).reshape(-1, 32))


def device_refine(ws, scene, cam=CAM, upload=True, jobs=None):
    """One sd_batch_relocalize_refine for the jobs of the scene -> [(result, frame_point (cap,), outlier (cap,))]; the per-stage
    downloads stay available on ws.b."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    jobs = scene["jobs"] if jobs is None else jobs
    n = len(jobs)
    kfp = np.full((max(n, 1), ws.cap), -1, np.int32); fp = np.full((max(n, 1), ws.cap), -1, np.int32)
    for q, j in enumerate(jobs):
        kfp[q, :len(j["kf_point"])] = j["kf_point"]; fp[q, :len(j["frame_point"])] = j["frame_point"]
    pts = np.ascontiguousarray(scene["points"], MP_DTYPE)
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda(); d_desc = torch.from_numpy(np.ascontiguousarray(scene["pdesc"], np.uint8).reshape(-1).copy()).cuda()
    d_kfp, d_fp = torch.from_numpy(kfp).cuda(), torch.from_numpy(fp).cuda()
    T = np.array([np.asarray(j["Tcw"], F32).reshape(16) for j in jobs], F32).reshape(n, 16)
    ws.b.relocalize_refine([j["frame"] for j in jobs], [j["kf"] for j in jobs], T, d_kfp.data_ptr(), d_fp.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(),
                           cam, n_points=len(pts))
    out = [ws.b.download_reloc(q) for q in range(n)]
    del d_pts, d_desc, d_kfp, d_fp
    return out


def found_of(kf_point, frame_point):
    """sFound over point ids -> the flag per keyframe feature."""
    ids = set(int(x) for x in frame_point if x >= 0)
    return np.array([1 if int(m) in ids else 0 for m in kf_point], np.uint8)


def check_stages(ws, scene, jobs, results, cam=CAM, quiet=False):
    """The last relocalize_refine of ws, stage by stage, so that a last-bit pose difference cannot pass for a matcher bug: every
    optimisation against the pose oracle on the device's own edges (n_good and outlier flags equal, pose within pose_close's 1e-5), every
    search byte for byte against the oracle matcher run from the device's own stage pose and assignment, and the assignment handed from
    step to step as lines 2311-2347 hand it."""
    import pose_cases as pc
    iv = fc.inv_sigma2(ws.lv)
    for q, j in enumerate(jobs):
        res, fp_final, out_final = results[q]
        Fk = scene["kfs"][j["frame"]]
        N2 = len(Fk["kp"])
        tag = "%s job %d" % (scene["name"], q)
        P = np.full(ws.cap, -1, np.int32); P[:N2] = j["frame_point"]
        O = np.zeros(ws.cap, np.uint8)
        T_prev = np.asarray(j["Tcw"], np.float32).reshape(4, 4)
        entry = P.copy()
        for k in range(3):
            edges, eo, Tin = ws.b.download_reloc_optimisation(q, k)
            ran = k == 0 or res["n_good"][k] >= 0
            if k > 0:                                             # the search between the optimisations
                w = k - 1
                pin, pout, frm, ex, best, nm = ws.b.download_reloc_search(q, w)
                assert pin.tobytes() == P.tobytes(), "%s: search %d does not start from the assignment the step before left" % (tag, w)
                if res["n_additional"][w] < 0:
                    assert pout.tobytes() == pin.tobytes() and nm == 0, tag
                else:
                    one = dict(scene, jobs=[dict(j, Tcw=res["Tcw_stage"][w], frame_point=pin[:N2], th=(10.0, 3.0)[w], orb=(100, 64)[w],
                                                 found=found_of(j["kf_point"], entry if w == 0 else pin))])
                    want, _ = cpu_search(one, cam=cam, lv=ws.lv)
                    assert_same(one, [(pout, frm, ex, best, nm)], want, "search %d of %s" % (w, tag))
                    assert nm == res["n_additional"][w]
                P = pout.copy()
            if not ran:
                assert len(edges) == 0 and res["Tcw_stage"][k].tobytes() == T_prev.tobytes(), tag
                continue
            idx = np.nonzero(P[:N2] >= 0)[0]
            assert list(edges["kp_index"]) == list(idx), "%s: optimisation %d: the edges are the assigned key points in order" % (tag, k)
            assert edges["xw"].tobytes() == scene["points"]["xw"][P[idx]].tobytes() and edges["u"].tobytes() == Fk["kp"]["x"][idx].tobytes()
            assert edges["v"].tobytes() == Fk["kp"]["y"][idx].tobytes() and edges["ur"].tobytes() == Fk["ur"][idx].tobytes()
            assert edges["inv_sigma2"].tobytes() == iv[Fk["kp"]["octave"][idx]].tobytes()
            assert Tin.tobytes() == T_prev.tobytes(), "%s: optimisation %d starts from the pose of the step before" % (tag, k)
            r, T, o, _ = pc.optimize(edges, cam, Tin)
            if not quiet:
                print("%s optimisation %d: n_good %d (oracle %d), |dT| %.2e" % (tag, k, res["n_good"][k], r, np.abs(T - res["Tcw_stage"][k]).max()))
            assert r == res["n_good"][k] and o.tobytes() == eo.tobytes(), "%s: optimisation %d: n_good %d vs %d" % (tag, k, res["n_good"][k], r)
            assert pc.pose_close(res["Tcw_stage"][k], T), "%s: optimisation %d: pose" % (tag, k)
            O[idx] = eo
            if (k == 0 and r >= 10) or k == 2:
                P[idx[eo != 0]] = -1
            T_prev = res["Tcw_stage"][k]
        assert fp_final.tobytes() == P.tobytes() and out_final.tobytes() == O.tobytes(), tag + ": the final assignment / mvbOutlier"
        assert res["Tcw"].tobytes() == res["Tcw_stage"][2].tobytes()
        ng = [x for x in res["n_good"] if x >= 0][-1]
        assert res["matched"] == (1 if ng >= 50 else 0)
        assert res["stage_reached"] == 1 + sum(1 for x in list(res["n_good"][1:]) + list(res["n_additional"]) if x >= 0)
