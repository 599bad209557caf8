"""Shared by test_proj_cases.py, test_gpu_proj.py and tools/fuzz_proj.py: crafted inputs for the two window matchers Tracking runs on
every frame -- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (k_proj_candidates / k_proj_resolve) and
Frame::isInFrustum + ORBmatcher::SearchByProjection(Frame, MapPoints, th) (k_local_candidates / k_local_resolve) -- that put a value ON
every decision edge of the two functions.  Plain numpy; the camera, the 640 x 480 grid of 10 x 10 pixel cells and the descriptor helpers
are area_cases' / fuse_cases'.

frame/frame   a PAIR is dict(name, cur, last (frames as fuse_cases' Workspace uploads them), xw, flags (the last frame's map points), Tcw,
              Tlw, occupied u8 [Nc], mpdesc (Nl, 32): a second descriptor array for d_mp_desc, cases [(case, point, outcome, key point)]);
              a scene is dict(name, th, bMono, pairs): one launch (or a few of at most four pairs: a pair takes two slots).
local map     a FRAME is dict(name, frame, points (MP_DTYPE), pdesc, Tcw, occupied, cases [(case, point, outcome, key point, extra)]);
              a scene is dict(name, th, nnratio, cos_limit, frames): one launch of up to eight frames.
np_search_by_projection / np_search_local_map restate both reference functions in numpy with f32 / f64 operations in the reference's
order: a second, independent statement that the CPU tests hold against the oracle on every scene of this file.
check_domain refuses what the contract does not cover (non-finite values, a NaN projection, octaves beyond the level set, counts above
the capacity); every upload goes through it.
Seeds depend on a case's kind and parameters only (the crc of its name), never on its place in a list."""
import zlib

import numpy as np

import area_cases as ac
import fuse_cases as fc
import triangulate_cases as tc
from triangulate_cases import F32, KP_DTYPE

CAM = ac.CAM
COLS, ROWS = ac.COLS, ac.ROWS
LV = tc.Levels()
NLEVELS = LV.nlevels
CAP = 600                     # key points per slot the scenes may use (the workspace's capacity is at least its nfeatures)
TH_HIGH = 100
HISTO = 30
TH_FF = 7.0                   # SearchByProjection(CurrentFrame, LastFrame, 7): radius 7 px at octave 0, 25.08 px at octave 7
I4 = np.eye(4, dtype=F32)
FF_OUTCOMES = ("no_point", "behind", "u_out", "v_out", "window_empty", "no_candidate", "dist>TH_HIGH", "matched", "matched_then_culled")
LM_OUTCOMES = ("flag_off", "behind", "u_out", "v_out", "dist_below_min", "dist_above_max", "view_angle", "window_empty", "no_candidate",
               "dist>TH_HIGH", "ratio", "matched")
POSE_A = tc.pose(tc.rodrigues([0.02, -0.03, 0.01]), [0.3, -0.2, 0.5]).astype(F32)
POSE_B = tc.pose(tc.rodrigues([-0.01, 0.015, 0.02]), [0.25, -0.15, 0.2]).astype(F32)


def _seed(name):
    return [20250, zlib.crc32(name.encode())]


def nextf(x, up=True):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


# ---------------------------------------------------------------- the kernels' f32 expressions in numpy
def mat3_mul_add(T, X):
    """R * x + t for (n, 3) f32 points: t = (a0*b0 + a1*b1) + a2*b2; d = t + c, every operation rounded to f32."""
    T = np.asarray(T, F32).reshape(4, 4); X = np.asarray(X, F32).reshape(-1, 3)
    out = np.zeros(X.shape, F32)
    with np.errstate(all="ignore"):
        for i in range(3):
            s = T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]
            s = s + T[i, 2] * X[:, 2]
            out[:, i] = s + T[i, 3]
    return out


def cam_centre(T):
    """-Rcw.t() * tcw in the same order."""
    T = np.asarray(T, F32).reshape(4, 4)
    o = np.zeros(3, F32)
    for i in range(3):
        s = (-T[0, i]) * T[0, 3] + (-T[1, i]) * T[1, 3]
        o[i] = s + (-T[2, i]) * T[2, 3]
    return o


def project_f32(T, X):
    """-> (u, v, invz, Xc): u = fx * xc * invz + cx with invz = 1.0f / zc."""
    Xc = mat3_mul_add(T, X)
    with np.errstate(all="ignore"):
        invz = F32(1.0) / Xc[:, 2]
        u = CAM["fx"] * Xc[:, 0] * invz + CAM["cx"]
        v = CAM["fy"] * Xc[:, 1] * invz + CAM["cy"]
    return u, v, invz, Xc


def back_project(T, u, v, z):
    """The world point (f32) that pose T sees near pixel (u, v) at depth z (computed in f64: `near`, not `at`)."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    Xc = np.array([(u - float(CAM["cx"])) / float(CAM["fx"]) * z, (v - float(CAM["cy"])) / float(CAM["fy"]) * z, z])
    return ((Xc - T[:3, 3]) @ T[:3, :3]).astype(F32)


def _roundf(x):
    """roundf on f32 values: half away from zero."""
    x = np.float64(x)
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


def _visiting(kp):
    """(px, py, in-grid key points in GetFeaturesInArea's visiting order: cells column-major, ascending index inside a cell)."""
    px, py = ac.cells(kp) if len(kp) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    idx = np.nonzero((px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS))[0]
    return px, py, idx[np.lexsort((idx, px[idx] * ROWS + py[idx]))]


def _area(kp, px, py, order, u, v, r, min_level, max_level):
    """Frame::GetFeaturesInArea in numpy -> indices in visiting order."""
    raw, (x0, x1, y0, y1) = ac.window(u, v, r)
    if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
        return []
    check = min_level > 0 or max_level >= 0
    out = []
    for j in order:
        if not (x0 <= px[j] <= x1 and y0 <= py[j] <= y1):
            continue
        o = int(kp["octave"][j])
        if check and (o < min_level or (max_level >= 0 and o > max_level)):
            continue
        if abs(kp["x"][j] - F32(u)) < F32(r) and abs(kp["y"][j] - F32(v)) < F32(r):
            out.append(int(j))
    return out


def three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(angle_last, angle_cur):
    rot = F32(angle_last) - F32(angle_cur)
    if rot < 0.0:
        rot = rot + F32(360.0)
    b = _roundf(rot * (F32(1.0) / F32(HISTO)))
    return 0 if b == HISTO else b


def tlc_z(Tcw, Tlw):
    return mat3_mul_add(Tlw, cam_centre(Tcw)[None])[0, 2]


def level_mode(Tcw, Tlw, bMono):
    z = tlc_z(Tcw, Tlw)
    return "forward" if (z > CAM["mb"] and not bMono) else "backward" if (-z > CAM["mb"] and not bMono) else "between"


def np_search_by_projection(P, th, bMono=False, check_orientation=True, use_mpdesc=False):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) restated -> dict(match, pairs, nm, outcome (names))."""
    cur, last = P["cur"], P["last"]
    kc, kl = cur["kp"], last["kp"]
    dmp = P["mpdesc"] if use_mpdesc else last["desc"]
    u, v, invz, _ = project_f32(P["Tcw"], P["xw"])
    mode = level_mode(P["Tcw"], P["Tlw"], bMono)
    px, py, order = _visiting(kc)
    taken = np.array(P["occupied"], bool).copy()
    match = np.full(len(kc), -1, np.int32); pairs = []; outcome = []
    bins = [[] for _ in range(HISTO)]
    for i in range(len(kl)):
        if not P["flags"][i] & 1:
            outcome.append("no_point"); continue
        if invz[i] < 0:
            outcome.append("behind"); continue
        if u[i] < CAM["mnMinX"] or u[i] > CAM["mnMaxX"]:
            outcome.append("u_out"); continue
        if v[i] < CAM["mnMinY"] or v[i] > CAM["mnMaxY"]:
            outcome.append("v_out"); continue
        o = int(kl["octave"][i])
        r = F32(th) * LV.scale[o]
        lo, hi = {"forward": (o, -1), "backward": (0, o), "between": (o - 1, o + 1)}[mode]
        members = _area(kc, px, py, order, u[i], v[i], r, lo, hi)
        if not members:
            outcome.append("window_empty"); continue
        best, bi = 256, -1
        for j in members:
            if taken[j]:
                continue
            if cur["ur"][j] > 0:
                ur = u[i] - CAM["mbf"] * invz[i]
                if abs(ur - cur["ur"][j]) > r:
                    continue
            d = int(ac.hamming(dmp[i], cur["desc"][j])[0])
            if d < best:
                best, bi = d, j
        if best <= TH_HIGH:
            match[bi] = i
            if P["flags"][i] & 2:
                taken[bi] = True
            pairs.append((i, bi))
            if check_orientation:
                bins[rot_bin(kl["angle"][i], kc["angle"][bi])].append((i, bi))
            outcome.append("matched")
        else:
            outcome.append("no_candidate" if bi < 0 else "dist>TH_HIGH")
    nm = len(pairs)
    if check_orientation:
        keep = three_maxima([len(b) for b in bins])
        for b in range(HISTO):
            if b not in keep:
                for i, bi in bins[b]:
                    match[bi] = -1; nm -= 1; outcome[i] = "matched_then_culled"
    return dict(match=match, pairs=np.array(pairs, np.int32).reshape(-1, 2), nm=nm, outcome=outcome)


def np_search_local_map(Fr, th, nnratio, cos_limit):
    """Frame::isInFrustum + ORBmatcher::SearchByProjection(F, MapPoints, th) restated -> dict(track fields, mp_match, kp_match, nm,
    outcome (names), best (M, 4))."""
    fr, pts = Fr["frame"], Fr["points"]
    kp = fr["kp"]; M = len(pts)
    T = np.asarray(Fr["Tcw"], F32)
    u, v, invz, Xc = project_f32(T, pts["xw"]) if M else (np.zeros(0, F32),) * 4
    Ow = cam_centre(T)
    logsf = F32(np.log(np.float64(LV.scale[1])))
    px, py, order = _visiting(kp)
    taken = np.array(Fr["occupied"], bool).copy()
    track = np.zeros(M, [("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"), ("in_view", "<i4")])
    outcome = [None] * M
    best4 = np.tile(np.array([256, 256, -1, -1], np.int32), (M, 1))
    for m in range(M):
        p = pts[m]
        if not p["flags"] & 1:
            outcome[m] = "flag_off"; continue
        if Xc[m, 2] < 0:
            outcome[m] = "behind"; continue
        if u[m] < CAM["mnMinX"] or u[m] > CAM["mnMaxX"]:
            outcome[m] = "u_out"; continue
        if v[m] < CAM["mnMinY"] or v[m] > CAM["mnMaxY"]:
            outcome[m] = "v_out"; continue
        po = p["xw"].astype(F32) - Ow
        s2 = 0.0
        for k in range(3):
            s2 += float(po[k]) * float(po[k])
        dist = F32(np.sqrt(s2))
        if dist < F32(0.8) * p["min_distance"]:
            outcome[m] = "dist_below_min"; continue
        if dist > F32(1.2) * p["max_distance"]:
            outcome[m] = "dist_above_max"; continue
        dot = 0.0
        for k in range(3):
            dot += float(po[k]) * float(p["normal"][k])
        vc = F32(dot / float(dist))
        if vc < F32(cos_limit):
            outcome[m] = "view_angle"; continue
        ratio = p["max_distance"] / dist
        n = int(np.ceil(F32(np.log(np.float64(ratio))) / logsf))
        n = 0 if n < 0 else min(n, NLEVELS - 1)
        track[m] = (u[m], v[m], u[m] - CAM["mbf"] * invz[m], vc, n, 1)
    nm = 0
    mpm = np.full(M, -1, np.int32); kpm = np.full(len(kp), -1, np.int32)
    for m in range(M):
        t, p = track[m], pts[m]
        if not t["in_view"]:
            continue
        r = F32(2.5) if float(t["view_cos"]) > 0.998 else F32(4.0)
        if F32(th) != 1.0:
            r = r * F32(th)
        lvl = int(t["level"])
        rad = r * LV.scale[lvl]
        members = _area(kp, px, py, order, t["proj_x"], t["proj_y"], rad, lvl - 1, lvl)
        if not members:
            outcome[m] = "window_empty"; continue
        b1, b2, l1, l2, bi = 256, 256, -1, -1, -1
        for j in members:
            if taken[j]:
                continue
            if fr["ur"][j] > 0 and abs(t["proj_xr"] - fr["ur"][j]) > rad:
                continue
            d = int(ac.hamming(Fr["pdesc"][m], fr["desc"][j])[0])
            if d < b1:
                b2, b1, l2, l1, bi = b1, d, l1, int(kp["octave"][j]), j
            elif d < b2:
                l2, b2 = int(kp["octave"][j]), d
        best4[m] = (b1, b2, l1, l2)
        outcome[m] = "no_candidate" if bi < 0 else "dist>TH_HIGH"
        if b1 <= TH_HIGH:
            if l1 == l2 and F32(b1) > F32(nnratio) * F32(b2):
                outcome[m] = "ratio"; continue
            kpm[bi] = m; mpm[m] = bi; nm += 1; outcome[m] = "matched"
            if p["flags"] & 2:
                taken[bi] = True
    return dict(track=track, mp_match=mpm, kp_match=kpm, nm=nm, outcome=outcome, best=best4)


# ---------------------------------------------------------------- the domain
def _finite(a, what):
    if not np.all(np.isfinite(np.asarray(a, np.float64))):
        raise ValueError("outside the domain: %s is not finite" % what)


def _check_frame(f, cap, what):
    k = f["kp"]
    if len(k) > cap:
        raise ValueError("outside the domain: %s holds %d key points, the capacity is %d" % (what, len(k), cap))
    if not (len(f["desc"]) == len(f["ur"]) == len(k)):
        raise ValueError("outside the domain: %s has arrays of different lengths" % what)
    for name in ("x", "y", "angle"):
        _finite(k[name], "%s key point %s" % (what, name))
    _finite(f["ur"], what + " uRight")
    if len(k) and (int(k["octave"].min()) < 0 or int(k["octave"].max()) >= NLEVELS):
        raise ValueError("outside the domain: %s has an octave outside the %d levels" % (what, NLEVELS))


def _check_projection(T, xw, live, what):
    _finite(T, what + " pose")
    _finite(xw, what + " world position")
    u, v, invz, _ = project_f32(T, xw)
    bad = live & ~(invz < 0) & (np.isnan(u) | np.isnan(v))
    if bad.any():
        raise ValueError("outside the domain: %s point %d projects to NaN (zc == 0 on an axis)" % (what, int(np.nonzero(bad)[0][0])))


def check_domain(obj, cap=CAP):
    """A pair, a local-map frame, or a scene of either; raises ValueError for what the contract does not cover."""
    if "pairs" in obj or "frames" in obj:
        for th in ("th",):
            if not (np.isfinite(obj[th]) and obj[th] > 0):
                raise ValueError("outside the domain: th")
        for o in obj.get("pairs", obj.get("frames")):
            check_domain(o, cap)
        return
    if "last" in obj:
        _check_frame(obj["cur"], cap, obj["name"] + ".cur"); _check_frame(obj["last"], cap, obj["name"] + ".last")
        n = len(obj["last"]["kp"])
        if not (len(obj["xw"]) == len(obj["flags"]) == n and len(obj["mpdesc"]) == n and len(obj["occupied"]) == len(obj["cur"]["kp"])):
            raise ValueError("outside the domain: %s has arrays of different lengths" % obj["name"])
        if n:
            _finite(obj["Tlw"], obj["name"] + " Tlw")
            _check_projection(obj["Tcw"], obj["xw"], (np.asarray(obj["flags"]) & 1) != 0, obj["name"])
        return
    _check_frame(obj["frame"], cap, obj["name"])
    pts = obj["points"]
    if len(pts) != len(obj["pdesc"]) or len(obj["occupied"]) != len(obj["frame"]["kp"]):
        raise ValueError("outside the domain: %s has arrays of different lengths" % obj["name"])
    if len(pts):
        for name in ("normal", "min_distance", "max_distance"):
            _finite(pts[name], "%s map point %s" % (obj["name"], name))
        live = (pts["flags"] & 1) != 0
        _check_projection(obj["Tcw"], pts["xw"], live, obj["name"])
        po = pts["xw"].astype(F32) - cam_centre(obj["Tcw"])
        if np.any(live & ~(np.abs(po).max(1) > 0)):
            raise ValueError("outside the domain: %s has a map point at the camera centre (viewCos is 0 / 0)" % obj["name"])
        if np.any(live & ~(pts["max_distance"] > 0)):
            raise ValueError("outside the domain: %s has a map point without mfMaxDistance (the scale ratio is not a positive number)" % obj["name"])


# ---------------------------------------------------------------- builders
def kp_rec(x, y, octave=0, angle=0.0):
    k = np.zeros((), KP_DTYPE)
    k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = x, y, 31.0, angle, 50.0, octave, -1
    return k


class FrameB:
    """Key points of one frame."""

    def __init__(self):
        self.k, self.d, self.ur, self.occ = [], [], [], []

    def add(self, x, y, desc, octave=0, ur=-1.0, angle=0.0, occupied=False):
        self.k.append(kp_rec(x, y, octave, angle)); self.d.append(np.asarray(desc, np.uint8).copy()); self.ur.append(F32(ur)); self.occ.append(1 if occupied else 0)
        return len(self.k) - 1

    def build(self):
        n = len(self.k)
        return dict(kp=np.array(self.k, KP_DTYPE) if n else np.zeros(0, KP_DTYPE), desc=np.array(self.d, np.uint8).reshape(n, 32),
                    ur=np.array(self.ur, F32).reshape(n), depth=np.full(n, -1, F32), Tcw=I4), np.array(self.occ, np.uint8).reshape(n)


class Lattice:
    """Window centres `step` pixels apart: with radii below step / 2 - 1 no window reaches a neighbour's key points."""

    def __init__(self, step, x0=None, y0=None):
        self.step, self.i = step, 0
        self.x0 = step // 2 + 10 if x0 is None else x0; self.y0 = step // 2 + 10 if y0 is None else y0
        self.nx = int((ac.W - 2 * self.x0) // step) + 1; self.ny = int((ac.H - 2 * self.y0) // step) + 1

    def next(self):
        i = self.i; self.i += 1
        assert i < self.nx * self.ny, "the lattice is full"
        return float(self.x0 + self.step * (i % self.nx)), float(self.y0 + self.step * (i // self.nx))


class PairB:
    """One frame pair of the frame/frame matcher."""

    def __init__(self, name, Tcw=I4, Tlw=I4, step=80):
        self.name, self.Tcw, self.Tlw = name, np.asarray(Tcw, F32), np.asarray(Tlw, F32)
        self.rng = np.random.default_rng(_seed(name))
        self.cur = FrameB(); self.lat = Lattice(step)
        self.lk, self.ld, self.xw, self.flags, self.alt, self.cases = [], [], [], [], {}, []

    def point(self, u=None, v=None, z=1.0, octave=0, desc=None, flags=3, angle=0.0, xw=None):
        """A last-frame map point that the current pose sees near (u, v) at depth z (or at xw exactly) -> its index."""
        if xw is None:
            if u is None:
                u, v = self.lat.next()
            xw = back_project(self.Tcw, u, v, z)
        self.lk.append(kp_rec(100.0, 100.0, octave, angle)); self.ld.append(fc.rand_desc(self.rng) if desc is None else np.asarray(desc, np.uint8).copy())
        self.xw.append(np.asarray(xw, F32)); self.flags.append(flags)
        return len(self.lk) - 1

    def uv(self, i):
        u, v, _, _ = project_f32(self.Tcw, self.xw[i])
        return u[0], v[0]

    def cand(self, i, dx, dy, bits, octave=None, **kw):
        """A current-frame key point at point i's projection + (dx, dy) whose descriptor is `bits` bits from the point's."""
        u, v = self.uv(i)
        return self.cur.add(F32(u + F32(dx)), F32(v + F32(dy)), fc.flipped(self.ld[i], bits, self.rng), int(self.lk[i]["octave"]) if octave is None else octave, **kw)

    def case(self, name, i, outcome, kp=-1):
        self.cases.append((name, i, outcome, kp))

    def simple(self, name, bits=10, outcome="matched", **kw):
        """A point with one candidate of its own 1 px away."""
        i = self.point(**kw); j = self.cand(i, 1.0, -1.0, bits)
        self.case(name, i, outcome, j if outcome.startswith("matched") else -1)
        return i, j

    def filler(self, n, flags=3, prefix="filler"):
        for _ in range(n):
            self.simple("%s_%d" % (prefix, len(self.lk)), bits=int(self.rng.integers(0, 60)), flags=flags)

    def build(self):
        n = len(self.lk)
        cur, occ = self.cur.build()
        last = dict(kp=np.array(self.lk, KP_DTYPE) if n else np.zeros(0, KP_DTYPE), desc=np.array(self.ld, np.uint8).reshape(n, 32),
                    ur=np.full(n, -1, F32), depth=np.full(n, -1, F32), Tcw=I4)
        mpdesc = last["desc"].copy()
        for i, d in self.alt.items():
            mpdesc[i] = d
        return dict(name=self.name, cur=cur, last=last, xw=np.array(self.xw, F32).reshape(n, 3), flags=np.array(self.flags, np.uint8).reshape(n),
                    Tcw=self.Tcw, Tlw=self.Tlw, occupied=occ, mpdesc=mpdesc, cases=self.cases)


def solve_xw(target, f, c):
    """x (f32) with fl(fl(f * x) + c) == target: the abscissa of a depth-1 point that the identity pose projects ONTO target."""
    return fc.solve_px(F32(target), f, c)


def _y_at(v):
    return F32((F32(v) - CAM["cy"]) / CAM["fy"])


def _x_at(u):
    return F32((F32(u) - CAM["cx"]) / CAM["fx"])


# ---------------------------------------------------------------- frame/frame: the named cases
def ff_bounds_pair():
    """Identity poses, depth 1: entry tests, inclusive image bounds, the radius in x, y and uRight at octaves 0 and 7, TH_HIGH, ties."""
    B = PairB("ff_bounds")
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    rng = B.rng
    # entry
    i = B.point(50.0, 440.0, flags=2); B.cand(i, 1.0, 0.0, 5); B.case("no_point", i, "no_point")
    i = B.point(xw=[0.1, 0.1, -1.0]); B.case("behind", i, "behind")
    i = B.point(xw=[0.3, 0.1, 0.0]); B.case("z_zero_plus", i, "u_out")            # invzc = +inf, u = +inf
    i = B.point(xw=[-0.3, 0.1, 0.0]); B.case("z_zero_minus", i, "u_out")          # u = -inf
    # image bounds: ON the bound is inside, one step of the world coordinate beyond it is outside
    for name, tu, tv, ku, kv in (("u_eq_minx", CAM["mnMinX"], 130.0, 3.0, 130.0), ("u_eq_maxx", CAM["mnMaxX"], 130.0, 634.0, 130.0),
                                 ("v_eq_miny", 290.0, CAM["mnMinY"], 290.0, 3.0), ("v_eq_maxy", 290.0, CAM["mnMaxY"], 290.0, 474.0)):
        x = solve_xw(tu, fx, cx) if name[0] == "u" else _x_at(tu)
        y = solve_xw(tv, fy, cy) if name[0] == "v" else _y_at(tv)
        i = B.point(xw=[x, y, 1.0])
        u, v = B.uv(i)
        assert (u == F32(tu)) if name[0] == "u" else (v == F32(tv)), name
        j = B.cur.add(ku, kv, fc.flipped(B.ld[i], 8, rng)); B.case(name, i, "matched", j)
        up = name.endswith(("maxx", "maxy"))
        xo, yo = x, y
        while True:                                                        # the first world coordinate whose projection leaves the image
            if name[0] == "u":
                xo = nextf(xo, up)
            else:
                yo = nextf(yo, up)
            k = B.point(xw=[xo, yo, 1.0], desc=B.ld[i]); uo, vo = B.uv(k)
            if (uo != u) or (vo != v):
                break
            B.lk.pop(); B.ld.pop(); B.xw.pop(); B.flags.pop()
        B.case(name.replace("_eq_", "_past_"), k, "u_out" if name[0] == "u" else "v_out")
    # the radius: |kp - projection| == radius is outside, one ulp nearer is inside; octave 0 (r = 7) and octave 7 (r = 7 * scale[7])
    for octave in (0, 7):
        r = F32(TH_FF) * LV.scale[octave]
        for axis in "xy":
            for which in ("on", "inside"):
                # each of the four has a point and a window of its own
                if octave == 7:                                            # windows of 25 px in the image's upper left part
                    pu, pv = {("x", "on"): (30.0, 30.0), ("x", "inside"): (30.0, 370.0), ("y", "on"): (130.0, 30.0), ("y", "inside"): (230.0, 30.0)}[(axis, which)]
                else:
                    pu, pv = {("x", "on"): (210.0, 210.0), ("x", "inside"): (210.0, 250.0), ("y", "on"): (250.0, 210.0), ("y", "inside"): (250.0, 250.0)}[(axis, which)]
                i = B.point(xw=[solve_xw(pu, fx, cx), solve_xw(pv, fy, cy), 1.0], octave=octave)
                u, v = B.uv(i)
                assert u == F32(pu) and v == F32(pv)
                sign = -1.0 if octave == 7 else 1.0                        # towards 0 where the difference is exact in f32
                edge = F32(pu + sign * r) if axis == "x" else F32(pv + sign * r)
                centre = F32(pu) if axis == "x" else F32(pv)
                assert abs(F32(edge - centre)) == r and np.float64(edge) - np.float64(centre) == sign * np.float64(r), "the edge key point is exactly r away"
                val = edge
                while which == "inside" and not abs(F32(val - centre)) < r:      # the first coordinate whose f32 DIFFERENCE is below r
                    val = nextf(val, up=sign < 0)
                j = B.cur.add(val if axis == "x" else pu + 1.0, val if axis == "y" else pv + 1.0, fc.flipped(B.ld[i], 9, rng), octave)
                B.case("radius_%s_oct%d_%s" % (axis, octave, which), i, "window_empty" if which == "on" else "matched", -1 if which == "on" else j)
        # stereo: ur = u - mbf * invzc = u - 40; |ur - uRight| == radius passes, one ulp more fails; uRight == 0 and < 0 skip the test
        pts = {0: ((370.0, 210.0), (370.0, 250.0), (410.0, 210.0), (410.0, 250.0), (450.0, 210.0)),
               7: ((30.0, 130.0), (30.0, 210.0), (30.0, 290.0), (130.0, 130.0), (130.0, 210.0))}[octave]
        for (pu, pv), which in zip(pts, ("on", "past", "on_low", "zero", "negative")):
            i = B.point(xw=[solve_xw(pu, fx, cx), _y_at(pv), 1.0], octave=octave)
            u, v = B.uv(i)
            urp = F32(u - CAM["mbf"] * F32(1.0))
            hi = F32(urp + r); lo = F32(urp - r)
            if which in ("on", "past", "on_low"):
                assert abs(F32(urp - hi)) == r and np.float64(hi) - np.float64(urp) == np.float64(r) and hi > 0
            past = nextf(hi)
            while not abs(F32(urp - past)) > r:                                # the first uRight whose f32 difference exceeds r
                past = nextf(past)
            ur = {"on": hi, "past": past, "on_low": lo if lo > 0 else hi, "zero": F32(0.0), "negative": F32(-3.0)}[which]
            j = B.cand(i, 1.0, 1.0, 12, ur=ur)
            B.case("uright_oct%d_%s" % (octave, which), i, "no_candidate" if which == "past" else "matched", -1 if which == "past" else j)
    # TH_HIGH
    i = B.point(50.0, 210.0); j = B.cand(i, 2.0, 0.0, 100); B.case("dist_100", i, "matched", j)
    B.alt[i] = tc._flip(B.cur.d[j], np.arange(101))                             # through d_mp_desc: 101, rejected
    i = B.point(50.0, 290.0); j = B.cand(i, 2.0, 0.0, 101); B.case("dist_101", i, "dist>TH_HIGH")
    B.alt[i] = tc._flip(B.cur.d[j], np.arange(100))                             # through d_mp_desc: 100, accepted
    # ties: the first VISITED wins, whatever its index.  Cell columns change at x = 10 k + 5.
    i = B.point(125.0, 370.0)
    a = B.cand(i, 3.0, 0.0, 20); b = B.cand(i, -3.0, 0.0, 20)                   # b: higher index, earlier column
    B.case("tie_2_later_index_first_cell", i, "matched", b)
    B.alt[i] = B.cur.d[a]                                                       # through d_mp_desc: a at distance 0
    i = B.point(225.0, 375.0)
    a = B.cand(i, 3.0, 3.0, 20); b = B.cand(i, -3.0, 3.0, 20); c = B.cand(i, -3.0, -3.0, 20)     # c: earliest column and row
    B.case("tie_3_cells", i, "matched", c)
    i = B.point(322.0, 372.0)
    a = B.cand(i, 1.0, 0.0, 20); b = B.cand(i, 0.0, 1.0, 20); c = B.cand(i, 1.0, 1.0, 20)        # one cell: the lowest index
    B.case("tie_3_one_cell", i, "matched", a)
    return B.build()


def ff_posed_pair():
    """Rotated and translated Tcw AND Tlw: every term of both products matters (the level mode is whatever tlc.z says)."""
    B = PairB("ff_posed", POSE_A, POSE_B, step=80)
    for k in range(12):
        z = float(B.rng.uniform(2.0, 30.0)); o = int(B.rng.integers(0, 8))
        i = B.point(z=z, octave=o)
        u, v = B.uv(i)
        stereo = k % 2 == 0
        _, _, invz, _ = project_f32(B.Tcw, B.xw[i])
        ur = F32(u - CAM["mbf"] * invz[0] + F32(B.rng.uniform(-3, 3))) if stereo else F32(-1)
        j = B.cand(i, float(B.rng.uniform(-4, 4)), float(B.rng.uniform(-4, 4)), int(B.rng.integers(0, 90)), ur=ur if ur > 0 or not stereo else -1.0)
        for q in (o - 2, o + 2):                                           # nearer descriptors no mode admits ... unless forward / backward does
            if 0 <= q < NLEVELS:
                B.cand(i, 2.0, 2.0, 3, octave=q)
        B.case("posed_%d" % k, i, None, None)                              # expectation: the numpy statement
    return B.build()


LEVEL_MODES = {"forward": -0.5, "backward": 0.5, "between": -0.05, "equal_mb": None}          # tz of Tcw = [I | (0, 0, tz)], Tlw = I: tlc.z = -tz


def allowed_octaves(mode, o):
    return {"forward": [q for q in range(NLEVELS) if q >= o], "backward": [q for q in range(NLEVELS) if q <= o],
            "between": [q for q in range(NLEVELS) if o - 1 <= q <= o + 1]}[mode]


def ff_level_pair(mode, bMono=False):
    """A pure z translation puts tlc.z above mb, below -mb, between them, or ON mb (strict >: not forward).  For last octaves 0, 3, 7 and
    each end of the admitted range one window with candidates at octaves o - 2 .. o + 2: the candidate just outside the range is the
    nearest (5 bits), the one just inside is next (10), the others lie at 40 and more."""
    tz = -CAM["mb"] if mode == "equal_mb" else F32(LEVEL_MODES[mode])
    T = I4.copy(); T[2, 3] = tz
    B = PairB("ff_level_" + mode + ("_mono" if bMono else ""), T, I4, step=80)
    z = tlc_z(T, I4)
    if mode == "equal_mb":
        assert z == CAM["mb"], "tlc.z equals mb bit for bit"
    eff = level_mode(T, I4, bMono)
    assert eff == ("between" if (mode == "equal_mb" or bMono) else mode)
    for o in (0, 3, 7):
        ok = [q for q in allowed_octaves(eff, o) if o - 2 <= q <= o + 2]
        for end in ("low", "high"):
            inside = ok[0] if end == "low" else ok[-1]
            outside = inside - 1 if end == "low" else inside + 1               # absent where the range has no such end among o - 2 .. o + 2
            i = B.point(z=2.0, octave=o)
            want = -1
            for n, q in enumerate(range(o - 2, o + 3)):
                if not 0 <= q < NLEVELS:
                    continue
                bits = 5 if q == outside else 10 if q == inside else 40 + n
                j = B.cand(i, float(n) - 2.0, 2.0 - float(n), bits, octave=q)
                if q == inside:
                    want = j
            B.case("level_%s%s_oct%d_%s" % (mode, "_mono" if bMono else "", o, end), i, "matched", want)
    return B.build()


def _contest(B, name, obs_first, second_for_b=True):
    """Points a then b prefer key point c (a: 5 bits, b: 6); b's second choice is d (30)."""
    a = B.point(flags=3 if obs_first else 1)
    c = B.cand(a, 1.0, 0.0, 0)
    b = B.point(xw=B.xw[a], desc=tc._flip(B.cur.d[c], [7, 100, 200, 31, 77, 150]), flags=3)
    B.ld[a] = tc._flip(B.cur.d[c], [1, 2, 3, 4, 5])
    d = B.cur.add(B.cur.k[c]["x"] + 2.0, B.cur.k[c]["y"] + 1.0, fc.flipped(B.ld[b], 30, B.rng)) if second_for_b else -1
    B.case(name + ".a", a, "matched", c)
    B.case(name + ".b", b, "matched" if (second_for_b or not obs_first) else "no_candidate", (d if obs_first else c))
    return a, b, c, d


def ff_order_pairs():
    """The assignment order: occupied key points, locks (flag bit 1), overwrites, the serial replay inside a 64-point chunk, contests
    across the 63 | 64 boundary, a chain; last-frame counts 0, 1, 63, 64, 65 and 70; an empty current frame."""
    out = []
    # 63 points: a lock and a chain (the replay path)
    B = PairB("ff_order63", step=40)
    B.filler(5)
    _contest(B, "lock", True)
    B.filler(3)
    a = B.point(flags=3); c = B.cand(a, 1.0, 0.0, 4)
    b = B.point(xw=B.xw[a], desc=fc.flipped(B.cur.d[c], 6, B.rng), flags=3)
    d = B.cur.add(B.cur.k[c]["x"] + 2.0, B.cur.k[c]["y"] + 1.0, fc.flipped(B.ld[b], 25, B.rng))
    B.filler(2)
    e = B.point(xw=B.xw[a], desc=fc.flipped(B.cur.d[d], 3, B.rng), flags=3)
    f = B.cur.add(B.cur.k[c]["x"] - 2.0, B.cur.k[c]["y"] - 1.0, fc.flipped(B.ld[e], 35, B.rng))
    B.case("chain.a", a, "matched", c); B.case("chain.b", b, "matched", d); B.case("chain.e", e, "matched", f)
    B.filler(63 - len(B.lk))
    out.append(B.build())
    # 64 points, none with observations: overwrites, committed in parallel; an occupied nearest candidate
    B = PairB("ff_order64", step=40)
    B.filler(7, flags=1)
    _contest(B, "overwrite", False)
    i = B.point(flags=1); j0 = B.cand(i, 1.0, 0.0, 5, occupied=True); j1 = B.cand(i, -1.0, 1.0, 20)
    B.case("occupied", i, "matched", j1)
    i = B.point(flags=1); B.cand(i, 1.0, 0.0, 5, occupied=True); B.case("occupied_only", i, "no_candidate")
    B.filler(64 - len(B.lk), flags=1)
    out.append(B.build())
    # 65 points: point 63 locks the key point that point 64 wants (no replay: the lock is visible at the next chunk's start)
    B = PairB("ff_order65", step=40)
    B.filler(63, flags=1)
    _contest(B, "boundary_lock", True)
    assert len(B.lk) == 65
    out.append(B.build())
    # 70 points (no multiple of 4 or 16): an overwrite across the boundary, then a lock inside the second chunk
    B = PairB("ff_order70", step=40)
    B.filler(63, flags=3)
    _contest(B, "boundary_overwrite", False)
    _contest(B, "lock_chunk1", True, second_for_b=False)
    B.filler(70 - len(B.lk))
    out.append(B.build())
    B = PairB("ff_order1", step=40); B.simple("single")
    out.append(B.build())
    B = PairB("ff_order0", step=40)
    for _ in range(5):
        u, v = B.lat.next(); B.cur.add(u, v, fc.rand_desc(B.rng))
    out.append(B.build())
    B = PairB("ff_cur_empty", step=40)
    for k in range(5):
        i = B.point(); B.case("cur_empty_%d" % k, i, "window_empty")
    out.append(B.build())
    return out


def _oriented(B, name, n, rot, flags=3, outcome="matched"):
    """n points whose match has rotation `rot` degrees (angle of the last key point - angle of the current one)."""
    out = []
    for k in range(n):
        al = float(B.rng.integers(0, 300)) if rot >= 0 else 10.0
        i = B.point(angle=al + max(rot, 0.0), flags=flags)
        j = B.cand(i, 1.0, 1.0, int(B.rng.integers(0, 50)), angle=al - min(rot, 0.0))
        B.case("%s_%d" % (name, k), i, outcome, j if outcome == "matched" else -1)
        out.append((i, j))
    return out


def ff_orientation_pairs():
    """Crafted key-point angles: the bins of the rotation histogram and ComputeThreeMaxima's strict comparisons."""
    out = []
    f = F32(1.0) / F32(HISTO)
    assert F32(15.0) * f == F32(0.5) and F32(135.0) * f == F32(4.5) and F32(45.0) * f > F32(1.5), "15 and 135 degrees land exactly on .5 (45: one ulp above)"
    for name, bins in (("hist_10_1", {0.0: (10, "matched"), 90.0: (1, "matched")}), ("hist_30_2", {0.0: (30, "matched"), 90.0: (2, "matched_then_culled")}),
                       ("hist_10_1_1", {0.0: (10, "matched"), 90.0: (1, "matched"), 150.0: (1, "matched")}),
                       ("hist_30_3_2", {0.0: (30, "matched"), 90.0: (3, "matched"), 150.0: (2, "matched_then_culled"), 240.0: (1, "matched_then_culled")}),
                       # rot = 15 -> bin 1 and rot = 45 -> bin 2 tie for first, rot = 135 -> bin 5 and bin 9 tie for third: the earlier bin
                       # wins (15 * (1/30) and 135 * (1/30) are exactly .5 in f32: halves round away from zero); rot = -30 -> 330 -> bin 11
                       ("hist_ties", {15.0: (5, "matched"), 45.0: (5, "matched"), 135.0: (2, "matched"), 270.0: (2, "matched_then_culled"),
                                      -30.0: (1, "matched_then_culled")}),
                       # rot == 0 stays in bin 0 (`rot < 0.0` is strict): were it moved to 360 it would join the ten of bin 12 and the
                       # single match of bin 3 would fall below a tenth
                       ("hist_rot_zero", {0.0: (10, "matched"), 350.0: (10, "matched"), 90.0: (1, "matched")}),
                       # 10 * (1/30) rounds down, 20 * (1/30) rounds up: truncated, both would share bin 0 and bin 3 would be culled
                       ("hist_round_not_truncate", {10.0: (10, "matched"), 20.0: (10, "matched"), 95.0: (1, "matched")}),
                       # 15 * (1/30) is exactly 0.5 and goes to bin 1 with rot = 31 (half away from zero); to even, bins 0 and 1 would hold
                       # ten each and the single match of bin 7 would survive
                       ("hist_half_away", {15.0: (10, "matched"), 31.0: (10, "matched"), 200.0: (1, "matched_then_culled")})):
        B = PairB("ff_" + name, step=40)
        for rot, (n, outcome) in bins.items():
            _oriented(B, "%s_rot%d" % (name, int(rot)), n, rot, outcome=outcome)
        out.append(B.build())
    for rot, b in ((15.0, 1), (45.0, 2), (135.0, 5), (-30.0, 11), (0.0, 0), (345.0, 12), (359.0, 12)):
        assert rot_bin(100.0 + rot if rot >= 0 else 10.0, 100.0 if rot >= 0 else 40.0) == b, rot
    # a culled pair whose key point a later point in a kept bin has taken: the key point's match is cleared although its owner survives
    B = PairB("ff_hist_cull_clears_owner", step=40)
    _oriented(B, "kept", 30, 0.0)
    a = B.point(angle=150.0, flags=1); c = B.cand(a, 1.0, 0.0, 5, angle=0.0)          # rot 150: bin 5, culled
    b = B.point(xw=B.xw[a], desc=fc.flipped(B.cur.d[c], 6, B.rng), angle=0.0, flags=3)  # rot 0: bin 0, kept; overwrites a's key point
    B.case("cull_clears.a", a, "matched_then_culled"); B.case("cull_clears.b", b, "matched", c)
    p = B.build(); p["cleared"] = c
    out.append(p)
    return out


def ff_scenes():
    """The named frame/frame cases -> [scene]; every scene is one call of the oracle per pair and a few launches of the device."""
    lv = [ff_level_pair(m) for m in LEVEL_MODES]
    return [dict(name="ff_geometry", th=TH_FF, bMono=False, pairs=[ff_bounds_pair(), ff_posed_pair()] + lv),
            dict(name="ff_mono", th=TH_FF, bMono=True, pairs=[ff_level_pair("forward", True), ff_level_pair("backward", True)]),
            dict(name="ff_order", th=TH_FF, bMono=False, pairs=ff_order_pairs()),
            dict(name="ff_orientation", th=TH_FF, bMono=False, pairs=ff_orientation_pairs())]


def nan_projection_pair():
    """zc == 0 with xc == 0: u = 0 * inf is NaN, passes every comparison of the bounds test and reaches the window: outside the domain."""
    B = PairB("ff_nan")
    i = B.point(xw=[0.0, 0.1, 0.0]); B.case("nan", i, None)
    return B.build()


# ---------------------------------------------------------------- local map: the named cases
class LocalB:
    """One frame and its local map points."""

    def __init__(self, name, Tcw=I4, step=80):
        self.name, self.Tcw = name, np.asarray(Tcw, F32)
        self.rng = np.random.default_rng(_seed(name))
        self.fr = FrameB(); self.lat = Lattice(step)
        self.pts, self.pd, self.cases = [], [], []

    def point(self, u=None, v=None, z=4.0, level=0, desc=None, flags=3, xw=None, normal=None, view_deg=0.0, min_distance=None, max_distance=None):
        """A map point seen near (u, v) at depth z, predicted at `level` (mfMaxDistance half a level above the distance), its normal
        view_deg degrees off the viewing ray."""
        if xw is None:
            if u is None:
                u, v = self.lat.next()
            xw = back_project(self.Tcw, u, v, z)
        xw = np.asarray(xw, F32)
        po = xw.astype(np.float64) - cam_centre(self.Tcw).astype(np.float64); dist = np.linalg.norm(po)
        r = np.zeros((), fc.MP_DTYPE)
        r["xw"] = xw
        if normal is None:
            ray = po / dist
            side = np.cross(ray, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
            normal = np.cos(np.radians(view_deg)) * ray + np.sin(np.radians(view_deg)) * side
        r["normal"] = normal
        mx = dist * 1.2 ** (level - 0.5) if max_distance is None else max_distance
        r["max_distance"] = mx
        r["min_distance"] = mx / float(LV.scale[-1]) if min_distance is None else min_distance
        r["flags"] = flags
        self.pts.append(r); self.pd.append(fc.rand_desc(self.rng) if desc is None else np.asarray(desc, np.uint8).copy())
        return len(self.pts) - 1

    def uv(self, m):
        u, v, _, _ = project_f32(self.Tcw, self.pts[m]["xw"])
        return u[0], v[0]

    def cand(self, m, dx, dy, bits, octave=0, **kw):
        u, v = self.uv(m)
        return self.fr.add(F32(u + F32(dx)), F32(v + F32(dy)), fc.flipped(self.pd[m], bits, self.rng), octave, **kw)

    def case(self, name, m, outcome, kp=-1, **extra):
        self.cases.append((name, m, outcome, kp, extra))

    def simple(self, name, bits=10, outcome="matched", level=0, octave=None, **kw):
        m = self.point(level=level, **kw); j = self.cand(m, 1.0, -1.0, bits, octave=level if octave is None else octave)
        self.case(name, m, outcome, j if outcome == "matched" else -1)
        return m, j

    def filler(self, n, flags=3):
        for _ in range(n):
            self.simple("filler_%d" % len(self.pts), bits=int(self.rng.integers(0, 60)), flags=flags)

    def build(self):
        n = len(self.pts)
        frame, occ = self.fr.build()
        return dict(name=self.name, frame=frame, points=np.array(self.pts, fc.MP_DTYPE) if n else np.zeros(0, fc.MP_DTYPE),
                    pdesc=np.array(self.pd, np.uint8).reshape(n, 32), Tcw=self.Tcw, occupied=occ, cases=self.cases)


def _on_bound(dist, factor, up):
    """m (f32) with fl(factor * m) == dist, and its neighbour on the rejecting side; None when the product skips dist."""
    m0 = F32(np.float64(dist) / np.float64(factor))
    for k in range(-4, 5):
        m = (m0.view(np.int32) + np.int32(k)).view(F32)
        if F32(factor) * m == dist:
            n = m
            while F32(factor) * n == dist:
                n = nextf(n, up)
            return m, n
    return None


def lm_frustum_frame(th, cos_limit):
    """Identity pose: the exits of Frame::isInFrustum with the value ON each bound, and one step beyond it."""
    B = LocalB("lm_frustum_%g_%g" % (th, cos_limit))
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
    m = B.point(50.0, 50.0, flags=2); B.cand(m, 0.5, 0.0, 5); B.case("flag_off", m, "flag_off")
    m = B.point(xw=[0.1, 0.1, -2.0], max_distance=2.0); B.case("behind", m, "behind")
    m = B.point(xw=[0.3, 0.1, 0.0], max_distance=0.3); B.case("z_zero", m, "u_out")
    for name, tu, tv, ku, kv in (("u_eq_minx", CAM["mnMinX"], 130.0, 1.0, 130.0), ("u_eq_maxx", CAM["mnMaxX"], 130.0, 634.5, 130.0),
                                 ("v_eq_miny", 290.0, CAM["mnMinY"], 290.0, 1.0), ("v_eq_maxy", 290.0, CAM["mnMaxY"], 290.0, 474.5)):
        x = solve_xw(tu, fx, cx) if name[0] == "u" else _x_at(tu)
        y = solve_xw(tv, fy, cy) if name[0] == "v" else _y_at(tv)
        m = B.point(xw=[x, y, 1.0], view_deg=8.0)                          # viewCos < 0.998: radius factor 4.0
        u, v = B.uv(m)
        assert (u == F32(tu)) if name[0] == "u" else (v == F32(tv)), name
        if th == 1.0 and name.endswith(("maxx", "maxy")):
            j = -1                                                         # radius 4: the last in-grid key point (< 635 / < 475) is out of reach
            B.case(name, m, "window_empty")
        else:
            j = B.fr.add(ku, kv, fc.flipped(B.pd[m], 8, B.rng)); B.case(name, m, "matched", j)
        up = name.endswith(("maxx", "maxy"))
        xo, yo = x, y
        while True:
            if name[0] == "u":
                xo = nextf(xo, up)
            else:
                yo = nextf(yo, up)
            k = B.point(xw=[xo, yo, 1.0], desc=B.pd[m]); uo, vo = B.uv(k)
            if (uo != u) or (vo != v):
                break
            B.pts.pop(); B.pd.pop()
        B.case(name.replace("_eq_", "_past_"), k, "u_out" if name[0] == "u" else "v_out")
    # dist == 0.8f * mfMinDistance and dist == 1.2f * mfMaxDistance: on the bound is inside
    for which, factor in (("min", F32(0.8)), ("max", F32(1.2))):
        found = None
        for z in (3.0, 3.3, 4.1, 5.2, 6.7, 2.3, 2.9, 7.9):
            xw = back_project(I4, 130.0 if which == "min" else 290.0, 210.0, z)
            dist = F32(np.sqrt(sum(float(c) * float(c) for c in xw)))
            found = _on_bound(dist, factor, up=(which == "min"))
            if found:
                break
        assert found, "no f32 %s distance whose product is the distance" % which
        on, past = found
        for tag, val in (("on", on), ("past", past)):
            kw = dict(min_distance=val, max_distance=float(dist)) if which == "min" else dict(max_distance=val, min_distance=0.1)
            m = B.point(xw=xw, **kw)
            if tag == "on":
                j = B.cand(m, 0.5, 0.5, 10, octave=0 if which == "max" else 0)
                # level: max / dist = 1 (min case) -> 0; 1 / 1.2 (max case) -> clamps to 0
                B.case("dist_%s_on" % which, m, "matched", j, level=0)
            else:
                B.pd[m] = B.pd[m - 1]
                B.case("dist_%s_past" % which, m, "dist_below_min" if which == "min" else "dist_above_max")
    # viewCos == viewingCosLimit: PO = (0, 0, z), |normal| irrelevant, viewCos = normal.z exactly
    lim = F32(cos_limit)
    for tag, nz in (("on", lim), ("past", nextf(lim, up=False))):
        m = B.point(xw=[0.0, 0.0, 2.0], normal=[0.3, 0.0, nz], desc=None if tag == "on" else B.pd[-1])
        if tag == "on":
            j = B.cand(m, 0.5, 0.5, 10); B.case("cos_limit_on", m, "matched", j)
        else:
            B.case("cos_limit_past", m, "view_angle")
    return B.build()


PATTERNS = {(5, 3, 5): (1, 0), (5, 5, 3): (2, 0), (5, 5, 4): (2, 0), (6, 5, 5): (1, 2), (4, 5, 5, 3): (3, 0)}     # -> (best, second) positions


def lm_levels_frame(th):
    """A rotated and translated pose: predicted levels, the radius factor, the level range."""
    B = LocalB("lm_levels_%g" % th, POSE_A, step=80)
    # PredictScale: mfMaxDistance / dist just below and just above 1.2^k; below 1 and above 1.2^7
    for k in (0, 1, 6, 7):
        for tag, q, want in (("below", 1.0 - 2e-4, k), ("above", 1.0 + 2e-4, min(k + 1, NLEVELS - 1))):
            u, v = B.lat.next()
            xw = back_project(B.Tcw, u, v, 3.0)
            dist = np.linalg.norm(xw.astype(np.float64) - cam_centre(B.Tcw).astype(np.float64))
            m = B.point(xw=xw, max_distance=dist * 1.2 ** k * q, min_distance=0.01)
            j = B.cand(m, 1.0, 1.0, 10, octave=want)
            B.case("level_1.2^%d_%s" % (k, tag), m, "matched", j, level=want)
    for tag, ratio, want in (("ratio_0.85", 0.85, 0), ("ratio_1.2^9", 1.2 ** 9, NLEVELS - 1)):
        u, v = B.lat.next()
        xw = back_project(B.Tcw, u, v, 3.0)
        dist = np.linalg.norm(xw.astype(np.float64) - cam_centre(B.Tcw).astype(np.float64))
        m = B.point(xw=xw, max_distance=dist * ratio, min_distance=0.01)
        j = B.cand(m, 1.0, 1.0, 10, octave=want)
        B.case("level_" + tag, m, "matched", j, level=want)
    # RadiusByViewingCos: a key point between 2.5 and 4.0 radii is reached only with viewCos <= 0.998 (f64 comparison of the f32 value)
    for tag, deg, outcome in (("cos_above_998", 3.0, "window_empty"), ("cos_below_998", 4.0, "matched")):
        m = B.point(level=0, view_deg=deg)
        j = B.cand(m, 3.2 * (th if th != 1.0 else 1.0), 0.0, 10)
        B.case("radius_factor_" + tag, m, outcome, j if outcome == "matched" else -1)
    # the level range [level - 1, level]: the candidate just outside is nearest
    for level in (3, 0):
        for end in ("low", "high"):
            inside = max(level - 1, 0) if end == "low" else level
            outside = inside - 1 if end == "low" else inside + 1
            m = B.point(level=level)
            want = -1
            for n, q in enumerate(range(level - 2, level + 2)):
                if q < 0 or (q != outside and q != inside):
                    continue
                j = B.cand(m, float(n) - 1.5, 1.5 - float(n), 5 if q == outside else 10, octave=q)
                if q == inside:
                    want = j
            B.case("levels_%d_%s" % (level, end), m, "matched", want)
    return B.build()


def lm_best_frame(th, nnratio):
    """Another pose: best / second best, the ratio test, an occupied nearest candidate, the stereo test."""
    B = LocalB("lm_best_%g_%g" % (th, nnratio), POSE_B, step=40)
    rng = B.rng
    # best / second best: distances (x 10) in VISITING order around a corner of four cells, indices in the opposite order
    for pat, (bp, sp) in PATTERNS.items():
        for split in (False, True):
            cu, cv = B.lat.next()
            cu, cv = 10.0 * round(cu / 10.0) + 5.0, 10.0 * round(cv / 10.0) + 5.0            # a corner of four cells
            m = B.point(cu, cv, level=1)
            pos = [(-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0)][:len(pat)]           # column-major visiting order
            u, v = B.uv(m)
            js = {}
            for n in reversed(range(len(pat))):
                octave = 0 if (split and n == sp) else 1
                js[n] = B.fr.add(F32(cu + pos[n][0]), F32(cv + pos[n][1]), fc.flipped(B.pd[m], 10 * pat[n], rng), octave)
            same = not split
            d0, d1 = 10 * pat[bp], 10 * pat[sp]
            rejected = same and F32(d0) > F32(nnratio) * F32(d1)
            B.case("pattern_%s_%s" % ("".join(map(str, pat)), "split" if split else "same"), m, "ratio" if rejected else "matched",
                   -1 if rejected else js[bp], best=(d0, d1, 1, 0 if split else 1))
    # the ratio ON the bound (same octave), a second best above TH_HIGH, and no second best
    for d0, d1 in ((25, 50), (26, 50), (40, 50), (41, 50), (90, 110), (100, None), (101, None)):
        m = B.point(level=0)
        j = B.cand(m, 1.0, 0.0, d0)
        if d1 is not None:
            B.cand(m, -1.0, 0.0, d1)
        rejected = d0 > TH_HIGH or (d1 is not None and F32(d0) > F32(nnratio) * F32(d1))
        B.case("ratio_%d_%s" % (d0, d1), m, ("dist>TH_HIGH" if d0 > TH_HIGH else "ratio") if rejected else "matched", -1 if rejected else j,
               best=(d0, 256 if d1 is None else d1, 0, -1 if d1 is None else 0))
    # the nearest candidate occupied: skipped BEFORE best and second are formed
    m = B.point(level=0)
    B.cand(m, 1.0, 0.0, 5, occupied=True); j = B.cand(m, -1.0, 0.0, 30); B.cand(m, 0.0, 1.0, 80)
    B.case("occupied_nearest", m, "matched", j, best=(30, 80, 0, 0))
    # stereo: |projXR - uRight| == radius passes, one ulp more fails (identity-free: the radius is exact, projXR is whatever f32 gives)
    for tag in ("on", "past"):
        m = B.point(level=0)
        u, v = B.uv(m)
        _, _, invz, _ = project_f32(B.Tcw, B.pts[m]["xw"])
        xr = F32(u - CAM["mbf"] * invz[0])
        rad = F32(2.5) * (F32(th) if th != 1.0 else F32(1.0))
        ur = None
        for cand in (F32(xr + rad), F32(xr - rad)):
            if cand > 0 and abs(F32(xr - cand)) == rad:
                ur = cand if tag == "on" else nextf(cand, up=cand > xr)
        assert ur is not None
        if tag == "past":
            assert abs(F32(xr - ur)) > rad
        j = B.cand(m, 0.5, 0.5, 10, ur=ur)
        B.case("uright_" + tag, m, "matched" if tag == "on" else "no_candidate", j if tag == "on" else -1)
    return B.build()


def _lm_contest(B, name, first_entry, obs):
    """a then b.  first_entry: b's best is the key point a takes; else it is b's SECOND best (same octave, fails the ratio while free)."""
    a = B.point(flags=3 if obs else 1)
    c = B.cand(a, 0.5, 0.0, 2)
    if first_entry:
        b = B.point(xw=B.pts[a]["xw"], desc=fc.flipped(B.fr.d[c], 10, B.rng), flags=3)
        d = B.fr.add(B.fr.k[c]["x"] - 1.0, B.fr.k[c]["y"] + 0.5, fc.flipped(B.pd[b], 60, B.rng), 0)
        # free: (10, 60) passes both ratios -> c; locked: d alone -> d
        B.case(name + ".a", a, "matched", c); B.case(name + ".b", b, "matched", d if obs else c)
    else:
        b = B.point(xw=B.pts[a]["xw"], flags=3)
        x = B.fr.add(B.fr.k[c]["x"] - 1.0, B.fr.k[c]["y"] + 0.5, fc.flipped(B.pd[b], 45, B.rng), 0)
        B.pd[b] = tc._flip(B.fr.d[x], np.arange(45))                       # b: x at 45, c at 50; a: c at 2
        B.fr.d[c] = tc._flip(B.pd[b], np.arange(100, 150))
        B.pd[a] = tc._flip(B.fr.d[c], [0, 1])
        # free: (45, 50) fails 0.5 and 0.8 -> ratio; c locked by a: x alone -> x
        B.case(name + ".a", a, "matched", c); B.case(name + ".b", b, "matched" if obs else "ratio", x if obs else -1)
    return a, b


def lm_order_frames(th):
    """The assignment order of the local-map search; 0, 1, 63, 64 and 65 points per frame."""
    out = []
    B = LocalB("lm_order63", POSE_B, step=40); B.filler(4)
    _lm_contest(B, "lock_first", True, True); B.filler(3); _lm_contest(B, "lock_second", False, True); B.filler(2)
    _lm_contest(B, "overwrite", True, False); _lm_contest(B, "free_second", False, False)
    B.filler(63 - len(B.pts)); out.append(B.build())
    B = LocalB("lm_order64_%g" % th, I4, step=40); B.filler(62, flags=1)
    # viewCos == (float)0.998 bit for bit: above 0.998 as a double (factor 2.5, the key point at 3.2 radii is out of reach), not above
    # 0.998f.  PO = (0, 0, 4) under the identity pose: viewCos = normal.z exactly.
    m = B.point(xw=[0.0, 0.0, 4.0], normal=[0.05, 0.0, F32(0.998)], flags=1)
    B.cand(m, 3.2 * th, 0.0, 10); B.case("cos_eq_998f", m, "window_empty")
    m = B.point(flags=1); j = B.cand(m, 0.5, 0.5, 10); B.case("last_of_64", m, "matched", j)
    assert len(B.pts) == 64
    out.append(B.build())
    B = LocalB("lm_order65", POSE_A, step=40); B.filler(63, flags=1); _lm_contest(B, "boundary_first", True, True)
    assert len(B.pts) == 65
    out.append(B.build())
    B = LocalB("lm_order65b", POSE_B, step=40); B.filler(63, flags=1); _lm_contest(B, "boundary_second", False, True)
    out.append(B.build())
    B = LocalB("lm_one", POSE_A, step=40); B.simple("single"); out.append(B.build())
    B = LocalB("lm_zero", POSE_B, step=40)                                 # no points: goes first, into the launch of eight
    for _ in range(4):
        u, v = B.lat.next(); B.fr.add(u, v, fc.rand_desc(B.rng))
    return [B.build()] + out


def lm_scenes():
    """The named local-map cases: th == 1.0 (no factor) with nnratio 0.5 and limit 0.5; th = 3 with 0.8 and 0.75.  Eight frames a launch,
    each with its own slot, offset and pose; one of them has no points (nine frames: a launch of eight and one of one)."""
    out = []
    for th, nn, lim in ((1.0, 0.5, 0.5), (3.0, 0.8, 0.75)):
        out.append(dict(name="lm_%g" % th, th=th, nnratio=nn, cos_limit=lim, frames=[lm_frustum_frame(th, lim), lm_levels_frame(th), lm_best_frame(th, nn)] + lm_order_frames(th)))
    return out


# ---------------------------------------------------------------- 1-ulp scans
FF_SCANS = ("u_maxx", "v_miny", "kpx_radius", "uright_radius")
LM_SCANS = ("u_minx", "min_distance", "max_distance", "cos_limit", "cos_998", "level_boundary", "kpy_radius")
SCAN_WINDOWS = 16
SCAN_TH_LM = 3.0


def walsh(i):
    """Row i of the 256 x 256 Hadamard matrix as a descriptor: any two rows differ in exactly 128 bits."""
    j = np.arange(256)
    bits = np.array([bin(int(i) & int(x)).count("1") & 1 for x in j], np.uint8)
    return np.packbits(bits, bitorder="little")


def _scan_z(variant):
    return 1.0 + 0.37 * variant


def _ff_scan_pairs(kind, items):
    """items [(variant, value)] -> scene; item k is point `where[k]` = (pair, index).  Four variants a pair.  The items of a variant share
    one projection; where a key point's coordinate slides every item has a key point and a Walsh descriptor of its own (128 bits from
    every other: only an item's own key point is within TH_HIGH)."""
    builders = [PairB("ff_scan_%s_%d" % (kind, q), step=40) for q in range(4)]
    where = []
    shared = {}
    for n, (variant, val) in enumerate(items):
        B = builders[variant // 4]
        z = _scan_z(variant)
        if kind == "u_maxx":
            vp = 20.0 + 28.0 * variant
            i = B.point(xw=[val, float(_y_at(vp)) * z, z], desc=walsh(1), flags=1)         # no observations: the shared key point stays free
            if variant not in shared:
                shared[variant] = B.cur.add(634.0, vp, tc._flip(walsh(1), [3, 9]))
        elif kind == "v_miny":
            up = 30.0 + 38.0 * variant
            i = B.point(xw=[float(_x_at(up)) * z, val, z], desc=walsh(1), flags=1)
            if variant not in shared:
                shared[variant] = B.cur.add(up, 3.0, tc._flip(walsh(1), [3, 9]))
        else:
            octave = variant % 3
            w = walsh(1 + len(B.lk))
            i = B.point(xw=back_project(I4, 60.0 + 150.0 * (variant % 4), 60.0 + 110.0 * (variant % 4), z), octave=octave, desc=w)
            u, v = B.uv(i)
            if kind == "kpx_radius":
                B.cur.add(val, v + F32(1.0), tc._flip(w, [3, 9, 200]), octave)
            else:
                B.cur.add(u + F32(1.0), v - F32(1.0), tc._flip(w, [3, 9, 200]), octave, ur=val)
        where.append((variant // 4, i))
    return dict(name="ff_scan_" + kind, th=TH_FF, bMono=False, pairs=[b.build() for b in builders]), where


def _ff_scan_start(kind, variant):
    """(an accepted value, a rejected one) of the sliding quantity."""
    z = _scan_z(variant)
    if kind == "u_maxx":
        return float(_x_at(636.0)) * z, float(_x_at(644.0)) * z
    if kind == "v_miny":
        return float(_y_at(4.0)) * z, float(_y_at(-4.0)) * z
    octave = variant % 3
    r = float(F32(TH_FF) * LV.scale[octave])
    u, v, invz, _ = project_f32(I4, back_project(I4, 60.0 + 150.0 * (variant % 4), 60.0 + 110.0 * (variant % 4), z))
    if kind == "kpx_radius":
        return float(u[0]) + r - 1.0, float(u[0]) + r + 1.0
    xr = float(u[0] - CAM["mbf"] * invz[0])
    return xr + r - 1.0, xr + r + 1.0


def _lm_scan_geometry(kind, variant):
    z = 2.0 + 0.41 * variant
    return 40.0 + 38.0 * variant, 30.0 + 28.0 * variant, z


def _scan_normal(po, kind):
    """A normal 60 degrees (cos_limit) or acos(0.998) (cos_998) off the viewing ray, and the component that slides: the one the ray is
    mostly along, kept well above 0."""
    deg = 60.0 if kind == "cos_limit" else np.degrees(np.arccos(0.998))
    ray = po / np.linalg.norm(po)
    axis = int(np.argmax(np.abs(ray)))
    side = np.cross(ray, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
    if side[axis] * ray[axis] < 0:
        side = -side
    n = np.cos(np.radians(deg)) * ray + np.sin(np.radians(deg)) * side
    return (n if ray[axis] > 0 else -n), axis


def _lm_scan_frames(kind, items):
    builders = [LocalB("lm_scan_%s_%d" % (kind, q), POSE_A if kind not in ("u_minx",) else I4, step=40) for q in range(4)]
    where, shared = [], {}
    for variant, val in items:
        B = builders[variant // 4]
        up, vp, z = _lm_scan_geometry(kind, variant)
        if kind == "u_minx":
            m = B.point(xw=[val, float(_y_at(vp)) * z, z], desc=walsh(1), flags=1)
            if variant not in shared:
                shared[variant] = B.fr.add(3.0, vp, tc._flip(walsh(1), [3, 9]))
        elif kind in ("min_distance", "max_distance", "cos_limit", "cos_998", "level_boundary"):
            xw = back_project(B.Tcw, up, vp, z)
            po = xw.astype(np.float64) - cam_centre(B.Tcw).astype(np.float64); dist = np.linalg.norm(po)
            octave = 0
            if kind == "min_distance":
                m = B.point(xw=xw, desc=walsh(1), min_distance=val, max_distance=dist, flags=1)
            elif kind == "max_distance":
                m = B.point(xw=xw, desc=walsh(1), max_distance=val, min_distance=0.01, flags=1)
            elif kind == "level_boundary":
                k = variant % 7
                octave = k + 1                                             # admitted at level k + 1 (and k + 2), not at level k
                m = B.point(xw=xw, desc=walsh(1), max_distance=val, min_distance=0.01, flags=1)
            else:
                nrm, axis = _scan_normal(po, kind)
                nrm = nrm.astype(F32); nrm[axis] = val
                m = B.point(xw=xw, desc=walsh(1), normal=nrm, flags=1)
            if variant not in shared:
                u, v = B.uv(m)
                dx = 3.2 * SCAN_TH_LM if kind == "cos_998" else 1.0
                shared[variant] = B.fr.add(F32(u + F32(dx)), v, tc._flip(walsh(1), [3, 9]), octave)
        else:                                                              # kpy_radius
            level = variant % 3
            w = walsh(1 + len(B.pts))
            m = B.point(xw=back_project(B.Tcw, 60.0 + 150.0 * (variant % 4), 60.0 + 110.0 * (variant % 4), z), level=level, desc=w)
            u, v = B.uv(m)
            B.fr.add(u + F32(1.0), val, tc._flip(w, [3, 9, 200]), level)
        where.append((variant // 4, m))
    return dict(name="lm_scan_" + kind, th=SCAN_TH_LM, nnratio=0.8, cos_limit=0.5, frames=[b.build() for b in builders]), where


def _lm_scan_start(kind, variant):
    up, vp, z = _lm_scan_geometry(kind, variant)
    if kind == "u_minx":
        return float(_x_at(4.0)) * z, float(_x_at(-4.0)) * z
    T = POSE_A
    if kind == "kpy_radius":
        xw = back_project(T, 60.0 + 150.0 * (variant % 4), 60.0 + 110.0 * (variant % 4), z)
        u, v, _, _ = project_f32(T, xw)
        r = 2.5 * SCAN_TH_LM * float(LV.scale[variant % 3])
        return float(v[0]) + r - 1.0, float(v[0]) + r + 1.0
    xw = back_project(T, up, vp, z)
    po = xw.astype(np.float64) - cam_centre(T).astype(np.float64); dist = np.linalg.norm(po)
    if kind == "min_distance":
        return dist / 0.9, dist / 0.7
    if kind == "max_distance":
        return dist / 1.1, dist / 1.3
    if kind == "level_boundary":
        k = variant % 7
        return dist * 1.2 ** k * 1.05, dist * 1.2 ** k * 0.95
    n, axis = _scan_normal(po, kind)
    assert n[axis] > 0.2
    if kind == "cos_limit":
        return float(n[axis]) + 0.05, float(n[axis]) - 0.05
    return float(n[axis]) - 0.02, float(n[axis]) + 0.02              # the key point between the radii is reached with viewCos <= 0.998


def scan_accepted(orc, scene, where):
    """Per item: matched, by the ORACLE."""
    if "pairs" in scene:
        res = [oracle_ff(orc, p, scene["th"], scene["bMono"]) for p in scene["pairs"]]
        code = FF_OUTCOMES.index("matched")
    else:
        res = [oracle_lm(orc, f, scene["th"], scene["nnratio"], scene["cos_limit"]) for f in scene["frames"]]
        code = LM_OUTCOMES.index("matched")
    return np.array([res[q]["outcome"][i] == code for q, i in where], bool)


_scan_cache = {}


def scan_scene(orc, kind, steps=512):
    """`steps` items in SCAN_WINDOWS windows: in each the sliding quantity takes consecutive f32 values centred on the bound `kind` names,
    for a geometry of its own.  The windows are placed by bisection with the ORACLE, all windows at once (one item each); the device
    never takes part.  -> (scene, where, variant of every item)."""
    if (kind, steps) in _scan_cache:
        return _scan_cache[(kind, steps)]
    W = SCAN_WINDOWS
    per = steps // W
    ff = kind in FF_SCANS
    build = (lambda it: _ff_scan_pairs(kind, it)) if ff else (lambda it: _lm_scan_frames(kind, it))
    start = [(_ff_scan_start if ff else _lm_scan_start)(kind, v) for v in range(W)]

    def accepted(vals):
        sc, where = build(list(enumerate(vals)))
        return scan_accepted(orc, sc, where)

    lo = np.array([s[0] for s in start], F32); hi = np.array([s[1] for s in start], F32)
    assert np.all(np.sign(lo) == np.sign(hi)) and np.all(lo != 0), "the bisection walks the integer view of floats of one sign"
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
    sc, where = build(items)
    _scan_cache[(kind, steps)] = (sc, where, np.array([v for v, _ in items]))
    return _scan_cache[(kind, steps)]


# ---------------------------------------------------------------- the truncated-list refusals
def _dense_members(B_add, u, v, n, base, octave=0, occupied=0, spread=5.0, rng=None):
    """n key points within `spread` px of (u, v); member k in VISITING order lies n - 1 - k bits from `base` (the last visited is the
    nearest); the `occupied` NEAREST ones are occupied."""
    x = u + rng.uniform(-spread, spread, n); y = v + rng.uniform(-spread, spread, n)
    probe = np.array([kp_rec(a, b, octave) for a, b in zip(x, y)], KP_DTYPE)
    px, py = ac.cells(probe)
    rank = np.empty(n, np.int64); rank[np.lexsort((np.arange(n), px * ROWS + py))] = np.arange(n)
    out = []
    for j in range(n):
        bits = n - 1 - int(rank[j])
        out.append(B_add(x[j], y[j], ac._prefix(base, bits), octave, occupied=bits < occupied))
    return out


def ff_refusal_pair(n, occupied):
    """One point over a window of n hits, the `occupied` nearest of them occupied, plus an ordinary point."""
    B = PairB("ff_refusal_%d_%d" % (n, occupied), step=80)
    i = B.point(320.0, 240.0)
    js = _dense_members(B.cur.add, 320.0, 240.0, n, B.ld[i], occupied=occupied, rng=B.rng)
    far = [j for j in js if not B.cur.occ[j]]
    B.case("dense", i, "matched" if far else "no_candidate", far[int(np.argmin([ac.hamming(B.ld[i], B.cur.d[j])[0] for j in far]))] if far else -1)
    B.simple("bystander", u=100.0, v=100.0)
    return B.build()


def lm_refusal_frame(n, occupied):
    B = LocalB("lm_refusal_%d_%d" % (n, occupied), I4, step=80)
    m = B.point(320.0, 240.0, level=0, flags=1)
    js = _dense_members(B.fr.add, 320.0, 240.0, n, B.pd[m], occupied=occupied, spread=5.0, rng=B.rng)
    B.case("dense", m, None, None)
    B.simple("bystander", u=100.0, v=100.0)
    return B.build()


REFUSAL_TH_LM = 3.0           # radius 7.5 px: the dense members lie within 5 px


# ---------------------------------------------------------------- seeded random scenes
def random_ff_scene(seed, n_pairs=4, n_points=220):
    """Random pairs: small rotations, forward / backward / sideways motion, random depths, octaves and flags, a share of occupied key
    points, mono and stereo key points, descriptors that are a few prototypes with flipped bits (ties and contests are common)."""
    rng = np.random.default_rng([777, seed])
    th = float(rng.choice([7.0, 10.0, 15.0])); bMono = bool(rng.random() < 0.25)
    pairs = []
    for q in range(n_pairs):
        Tl = tc.pose(tc.rodrigues(rng.normal(size=3) * 0.02), rng.normal(size=3) * 0.1).astype(F32)
        motion = [(0, 0, 0.4), (0, 0, -0.4), (0.3, 0.0, 0.02), (0.0, 0.0, 0.0)][int(rng.integers(0, 4))]
        Tc = tc.neighbour_pose(Tl.astype(np.float64), motion, rng.normal(size=3) * 0.01).astype(F32)
        B = PairB("ff_random_%d_%d" % (seed, q), Tc, Tl)
        B.rng = rng
        protos = [fc.rand_desc(rng) for _ in range(6)]
        n = int(rng.integers(n_points // 2, n_points))
        for _ in range(n):
            u, v = float(rng.uniform(-8, 648)), float(rng.uniform(-8, 488)); z = float(rng.uniform(0.8, 30.0))
            o = int(rng.integers(0, NLEVELS))
            pr = int(rng.integers(0, 6))
            i = B.point(u, v, z if rng.random() > 0.03 else -z, octave=o, desc=fc.flipped(protos[pr], int(rng.integers(0, 40)), rng),
                        flags=int(rng.choice([0, 1, 1, 3, 3, 3, 3, 3])), angle=float(rng.choice([0.0, 0.0, 10.0, 15.0, 45.0, 200.0, 340.0])))
            for _ in range(int(rng.integers(0, 5))):
                uu, vv = B.uv(i)
                if not (np.isfinite(uu) and np.isfinite(vv)):
                    continue
                s = float(LV.scale[o])
                kx, ky = float(uu) + rng.normal() * 0.35 * th * s, float(vv) + rng.normal() * 0.35 * th * s
                stereo = rng.random() < 0.6
                _, _, invz, _ = project_f32(B.Tcw, B.xw[i])
                ur = float(uu - CAM["mbf"] * invz[0]) + rng.normal() * 0.5 * th * s if stereo else -1.0
                kpr = pr if rng.random() < 0.75 else int(rng.integers(0, 6))
                B.cur.add(kx, ky, fc.flipped(protos[kpr], int(rng.integers(0, 60)), rng), int(np.clip(o + rng.integers(-2, 3), 0, NLEVELS - 1)),
                          ur=ur if np.isfinite(ur) else -1.0, angle=float(rng.choice([0.0, 10.0, 30.0, 200.0])), occupied=rng.random() < 0.1)
                if len(B.cur.k) >= CAP:
                    break
            if len(B.cur.k) >= CAP:
                break
        pairs.append(B.build())
    return dict(name="ff_random_%d" % seed, th=th, bMono=bMono, pairs=pairs)


def random_lm_scene(seed, n_frames=4, n_points=260):
    rng = np.random.default_rng([778, seed])
    th = float(rng.choice([1.0, 3.0, 5.0])); nn = float(rng.choice([0.5, 0.8])); lim = float(rng.choice([0.5, 0.7]))
    frames = []
    for q in range(n_frames):
        T = tc.pose(tc.rodrigues(rng.normal(size=3) * 0.03), rng.normal(size=3) * 0.2).astype(F32)
        B = LocalB("lm_random_%d_%d" % (seed, q), T)
        B.rng = rng
        protos = [fc.rand_desc(rng) for _ in range(6)]
        n = int(rng.integers(n_points // 2, n_points))
        for _ in range(n):
            u, v = float(rng.uniform(-8, 648)), float(rng.uniform(-8, 488)); z = float(rng.uniform(0.8, 30.0))
            level = int(rng.integers(0, NLEVELS))
            xw = back_project(T, u, v, z if rng.random() > 0.03 else -z)
            dist = np.linalg.norm(xw.astype(np.float64) - cam_centre(T).astype(np.float64))
            pr = int(rng.integers(0, 6))
            lim_deg = float(np.degrees(np.arccos(lim)))
            m = B.point(xw=xw, desc=fc.flipped(protos[pr], int(rng.integers(0, 40)), rng), flags=int(rng.choice([0, 1, 1, 3, 3, 3, 3, 3])),
                        view_deg=float(rng.choice([0.0, 0.0, 3.0, 3.6, 3.7, 4.0, 30.0, lim_deg - 1.0, lim_deg + 1.0])),
                        max_distance=dist * 1.2 ** level * float(rng.uniform(0.8, 1.25)))
            B.pts[m]["min_distance"] = B.pts[m]["max_distance"] / F32(1.2 ** 7) * F32(rng.uniform(0.5, 1.3))
            uu, vv = B.uv(m)
            if not (np.isfinite(uu) and np.isfinite(vv)):
                continue
            for _ in range(int(rng.integers(0, 5))):
                o = int(np.clip(level + rng.integers(-2, 2), 0, NLEVELS - 1))
                s = float(LV.scale[level]) * th
                stereo = rng.random() < 0.6
                _, _, invz, _ = project_f32(T, xw)
                ur = float(uu - CAM["mbf"] * invz[0]) + rng.normal() * 1.5 * s if stereo else -1.0
                kpr = pr if rng.random() < 0.75 else int(rng.integers(0, 6))
                B.fr.add(float(uu) + rng.normal() * 1.2 * s, float(vv) + rng.normal() * 1.2 * s, fc.flipped(protos[kpr], int(rng.integers(0, 60)), rng),
                         o, ur=ur if np.isfinite(ur) else -1.0, occupied=rng.random() < 0.1)
                if len(B.fr.k) >= CAP:
                    break
            if len(B.fr.k) >= CAP:
                break
        frames.append(B.build())
    return dict(name="lm_random_%d" % seed, th=th, nnratio=nn, cos_limit=lim, frames=frames)


# ---------------------------------------------------------------- the oracle and the device
def oracle_ff(orc, P, th, bMono, check_orientation=True, use_mpdesc=False):
    cur, last = P["cur"], P["last"]
    m, pairs, nm, out = orc.search_by_projection_ex(cur["kp"], cur["desc"], cur["ur"], last["kp"], P["mpdesc"] if use_mpdesc else last["desc"], P["xw"],
                                                     P["flags"], P["Tcw"], P["Tlw"], ac.cam_array(), LV.scale, th, bMono, check_orientation,
                                                     occupied=P["occupied"] if len(P["occupied"]) else None)
    return dict(match=m, pairs=pairs, nm=nm, outcome=out)


def oracle_lm(orc, Fr, th, nnratio, cos_limit):
    fr = Fr["frame"]
    tr, pm, km, nm, out, best = orc.search_local_map_ex(fr["kp"], fr["desc"], fr["ur"], np.ascontiguousarray(Fr["points"]).view(orc.MAP_POINT_DTYPE), Fr["pdesc"],
                                                        Fr["Tcw"], ac.cam_array(), LV.scale, th, nnratio, cos_limit,
                                                        occupied=Fr["occupied"] if len(Fr["occupied"]) else None)
    return dict(track=tr, mp_match=pm, kp_match=km, nm=nm, outcome=out, best=best)


def upload(ws, frames, first=0):
    """Frames over slots first ..; the grid is assigned for every slot up to the last one written."""
    for f in frames:
        _check_frame(f, ws.cap, "upload")
    ws.upload(frames, first=first)
    ws.b.assign_grid(first + len(frames), CAM)
    ws.b.sync()


def device_ff(ws, scene, pairs=None, check_orientation=True, use_mpdesc=False, jobs=None, do_upload=True):
    """The pairs of a scene on the device, four pairs (eight slots) a launch -> [dict(match, pairs, nm)] per pair.
    jobs: [(pair, last slot, cur slot)] run as ONE launch on frames already uploaded (do_upload = False)."""
    import torch
    pairs = scene["pairs"] if pairs is None else pairs
    out = []
    groups = [[(P, 2 * k, 2 * k + 1) for k, P in enumerate(pairs[g:g + 4])] for g in range(0, len(pairs), 4)] if jobs is None else [jobs]
    for group in groups:
        for P, _, _ in group:
            check_domain(P, ws.cap)
        if do_upload:
            fr = [None] * (2 * len(group))
            for P, ls, cs in group:
                fr[ls], fr[cs] = P["last"], P["cur"]
            upload(ws, fr)
        n = len(group)
        occ = np.zeros((n, ws.cap), np.uint8)
        mpd = np.zeros((ws.n, ws.cap, 32), np.uint8)
        for q, (P, ls, cs) in enumerate(group):
            if len(P["xw"]):
                ws.b.set_mappoints(ls, P["xw"], P["flags"])
            occ[q, :len(P["occupied"])] = P["occupied"]
            mpd[ls, :len(P["mpdesc"])] = P["mpdesc"]
        d_occ = torch.from_numpy(occ).cuda()
        d_mpd = torch.from_numpy(mpd).cuda() if use_mpdesc else None
        ws.b.search_by_projection([g[2] for g in group], [g[1] for g in group], np.array([g[0]["Tcw"] for g in group], F32), np.array([g[0]["Tlw"] for g in group], F32),
                                  CAM, scene["th"], scene["bMono"], check_orientation, d_occupied=d_occ.data_ptr(),
                                  d_mp_desc=d_mpd.data_ptr() if use_mpdesc else None)
        ws.b.sync()
        for q, (P, ls, cs) in enumerate(group):
            m, pr, nm = ws.b.download_matches(q)
            out.append(dict(match=m[:len(P["cur"]["kp"])].copy(), pairs=pr, nm=nm))
        del d_occ, d_mpd
    return out


def device_lm(ws, scene, frames=None, slots=None, do_upload=True):
    """The frames of a scene in ONE launch (frame q on slot slots[q], default q) -> [dict(track, mp_match, kp_match, nm)] per frame."""
    import torch
    frames = scene["frames"] if frames is None else frames
    if slots is None and len(frames) > ws.n:
        return device_lm(ws, scene, frames[:ws.n]) + device_lm(ws, scene, frames[ws.n:])
    slots = list(range(len(frames))) if slots is None else slots
    for F in frames:
        check_domain(F, ws.cap)
    if do_upload:
        fr = [dict(kp=np.zeros(0, KP_DTYPE), desc=np.zeros((0, 32), np.uint8), ur=np.zeros(0, F32), depth=np.zeros(0, F32))] * (max(slots) + 1)
        fr = list(fr)
        for F, s in zip(frames, slots):
            fr[s] = F["frame"]
        upload(ws, fr)
    off = np.concatenate([[0], np.cumsum([len(F["points"]) for F in frames])]).astype(np.int32)
    M = int(off[-1])
    pts = np.concatenate([np.ascontiguousarray(F["points"], fc.MP_DTYPE) for F in frames]) if M else np.zeros(1, fc.MP_DTYPE)
    pd = np.concatenate([F["pdesc"] for F in frames]) if M else np.zeros((1, 32), np.uint8)
    occ = np.zeros((len(frames), ws.cap), np.uint8)
    for q, F in enumerate(frames):
        occ[q, :len(F["occupied"])] = F["occupied"]
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda(); d_pd = torch.from_numpy(np.ascontiguousarray(pd).copy()).cuda()
    d_occ = torch.from_numpy(occ).cuda()
    d_track = torch.zeros(max(M, 1) * 24, dtype=torch.uint8, device="cuda"); d_pm = torch.full((max(M, 1),), -7, dtype=torch.int32, device="cuda")
    d_km = torch.full((len(frames), ws.cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
    ws.b.search_local_map(slots, off, d_pts.data_ptr(), d_pd.data_ptr(), np.array([F["Tcw"] for F in frames], F32), CAM, scene["th"], scene["nnratio"],
                          d_track.data_ptr(), d_pm.data_ptr(), d_km.data_ptr(), d_nm.data_ptr(), viewing_cos_limit=scene["cos_limit"], d_occupied=d_occ.data_ptr())
    ws.b.sync()
    track = d_track.cpu().numpy(); pm = d_pm.cpu().numpy(); km = d_km.cpu().numpy(); nm = d_nm.cpu().numpy()
    out = []
    for q, F in enumerate(frames):
        out.append(dict(track=track[24 * off[q]:24 * off[q + 1]].copy(), mp_match=pm[off[q]:off[q + 1]].copy(), kp_match=km[q, :len(F["frame"]["kp"])].copy(), nm=int(nm[q])))
    del d_pts, d_pd, d_occ, d_track, d_pm, d_km, d_nm
    return out


def histogram(outcomes, names):
    """{name: count} of the outcome codes, in exit order."""
    c = np.bincount(np.asarray(outcomes, np.int64), minlength=len(names)) if len(outcomes) else np.zeros(len(names), np.int64)
    return {n: int(k) for n, k in zip(names, c) if k}


def same_ff(got, want, what):
    """Bytes of match[:Nc], pairs and nmatches."""
    assert got["nm"] == want["nm"], "%s: nmatches %d vs %d" % (what, got["nm"], want["nm"])
    assert np.asarray(got["pairs"], np.int32).tobytes() == np.asarray(want["pairs"], np.int32).tobytes(), "%s: pairs differ" % what
    assert np.asarray(got["match"], np.int32).tobytes() == np.asarray(want["match"], np.int32).tobytes(), \
        "%s: match differs at key points %r" % (what, np.nonzero(np.asarray(got["match"]) != np.asarray(want["match"]))[0][:8])


def same_lm(got, want, what):
    """Bytes of the track records (floats as their bits), point_match, kp_match[:N] and nmatches."""
    g = np.frombuffer(np.asarray(got["track"]).tobytes(), np.uint32).reshape(-1, 6); w = np.frombuffer(np.asarray(want["track"]).tobytes(), np.uint32).reshape(-1, 6)
    assert g.shape == w.shape and np.array_equal(g, w), "%s: track records differ at points %r" % (what, np.nonzero((g != w).any(1))[0][:8])
    assert got["nm"] == want["nm"], "%s: nmatches %d vs %d" % (what, got["nm"], want["nm"])
    assert np.array_equal(got["mp_match"], want["mp_match"]), "%s: point_match differs at %r" % (what, np.nonzero(got["mp_match"] != want["mp_match"])[0][:8])
    assert np.array_equal(got["kp_match"], want["kp_match"]), "%s: kp_match differs" % what
