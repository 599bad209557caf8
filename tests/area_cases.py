"""Shared by test_area_cases.py and test_gpu_area.py: one crafted frame pair on a 640 x 480 camera that pins the seams of the window
walk the projection matchers share (csrc/k_area.h) -- the hand-over from a group of 16 lanes to the whole wave in k_proj_candidates
(a window of 16 / 17 grid columns, 16 / 17 hits), the flush of the 64-key row into the running best-64 (64 / 65 hits, in
k_proj_candidates and k_local_candidates) and windows the image borders clip.  Plain numpy.

The poses are the identity and every point lies at depth 1, so a point projects where the f32 expression of the kernels puts it
(project()).  The grid cells are 10 x 10 pixels.  A window's members are current-frame key points placed for it alone: no two
windows with different centres share a cell.  Last-frame point i carries key point i of the last frame (its octave sets the radius
th * scale[octave]) and descriptor i; the local-map points carry their own records and descriptors.

A dense window of n members is searched by two points.  Member k in VISITING order holds the base descriptor with its first
n - 1 - k bits inverted: to point A (the base) every distance is distinct and each member visited later is nearer, so the last one
visited -- beyond the 64-key row when n = 65 -- is the best.  To point B (the base with the even bits of its first 128 inverted)
the members lie at 63 and 64 bits alternately: ties that only the visiting order breaks."""
import numpy as np

import fuse_cases as fc
import triangulate_cases as tc
from triangulate_cases import F32, KP_DTYPE

W, H = 640, 480
COLS, ROWS = 64, 48
CAM = dict(fx=F32(520.0), fy=F32(520.0), cx=F32(320.5), cy=F32(240.5), mbf=F32(40.0))
CAM["mb"] = F32(CAM["mbf"] / CAM["fx"])
CAM.update(mnMinX=F32(0), mnMaxX=F32(W), mnMinY=F32(0), mnMaxY=F32(H))
TH_PROJ = 20.0            # SearchByProjection(CurrentFrame, LastFrame, th): radius 20 px at octave 0, 71.66 px at octave 7
TH_LOCAL = 8.0            # SearchByProjection(Frame, MapPoints, th): radius 2.5 * 8 * scale[0] = 20 px
TH_HIGH = 100
IDENTITY = np.eye(4, dtype=F32)
DENSE = ((16, 63.0), (17, 163.0), (64, 263.0), (65, 363.0))          # (members, u of the centre); v = 403


def cam_array():
    return fc.cam_array(CAM)


def point_at(u, v):
    """The world point at depth 1 that the identity pose sees near pixel (u, v)."""
    return np.array([(F32(u) - CAM["cx"]) / CAM["fx"], (F32(v) - CAM["cy"]) / CAM["fy"], 1.0], F32)


def project(xw):
    """(u, v) of (n, 3) f32 points under the identity pose, in the kernels' f32 order: fx * xc * invz + cx."""
    xw = np.asarray(xw, F32).reshape(-1, 3)
    invz = F32(1.0) / xw[:, 2]
    return CAM["fx"] * xw[:, 0] * invz + CAM["cx"], CAM["fy"] * xw[:, 1] * invz + CAM["cy"]


def grid_inv():
    return F32(COLS) / (CAM["mnMaxX"] - CAM["mnMinX"]), F32(ROWS) / (CAM["mnMaxY"] - CAM["mnMinY"])


def window(u, v, r):
    """GetFeaturesInArea's cell bounds in f32 -> (unclamped (x0, x1, y0, y1), clamped (x0, x1, y0, y1))."""
    wi, hi = grid_inv()
    u, v, r = F32(u), F32(v), F32(r)
    raw = (int(np.floor((u - CAM["mnMinX"] - r) * wi)), int(np.ceil((u - CAM["mnMinX"] + r) * wi)),
           int(np.floor((v - CAM["mnMinY"] - r) * hi)), int(np.ceil((v - CAM["mnMinY"] + r) * hi)))
    return raw, (max(0, raw[0]), min(COLS - 1, raw[1]), max(0, raw[2]), min(ROWS - 1, raw[3]))


def cells(kp):
    """Frame::PosInGrid in f32 -> (column, row) per key point (roundf: half away from zero; nothing here is negative)."""
    wi, hi = grid_inv()
    px = np.floor(((kp["x"] - CAM["mnMinX"]) * wi).astype(np.float64) + 0.5).astype(np.int64)
    py = np.floor(((kp["y"] - CAM["mnMinY"]) * hi).astype(np.float64) + 0.5).astype(np.int64)
    return px, py


def hamming(a, B):
    return np.unpackbits(np.asarray(a, np.uint8)[None, :] ^ np.asarray(B, np.uint8).reshape(-1, 32), axis=1).sum(1).astype(np.int64)


def walk(kp, u, v, r):
    """What the device's walk hands out for the window (u, v, r): dict(span = grid columns, clipped = the borders that cut it,
    order = the members' indices in visiting order (column-major cells, ascending index inside a cell))."""
    raw, (x0, x1, y0, y1) = window(u, v, r)
    px, py = cells(kp)
    inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (px < COLS) & (py < ROWS)
    idx = np.nonzero(inside)[0]
    order = idx[np.lexsort((idx, px[idx] * ROWS + py[idx]))]
    clipped = {name for name, cut in (("left", raw[0] < 0), ("right", raw[1] > COLS - 1), ("top", raw[2] < 0), ("bottom", raw[3] > ROWS - 1)) if cut}
    return dict(span=x1 - x0 + 1, clipped=clipped, order=order, first_col=x0, last_col=x1, cols=px[order])


def in_radius(kp, order, u, v, r):
    k = kp[order]
    return (np.abs(k["x"] - F32(u)) < F32(r)) & (np.abs(k["y"] - F32(v)) < F32(r))


def _kp(x, y, octave):
    k = np.zeros((), KP_DTYPE)
    k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = x, y, 31.0, 0.0, 50.0, octave, -1
    return k


def _prefix(base, n):
    """`base` with its first n bits inverted."""
    return tc._flip(np.asarray(base, np.uint8), np.arange(n))


def _alternate(base):
    """`base` with the even bits of its first 128 inverted."""
    return tc._flip(np.asarray(base, np.uint8), np.arange(0, 128, 2))


def scene():
    """-> dict(last, cur: frames as fuse_cases' Workspace uploads them; xw (n, 3) f32, flags u8: the last frame's map points;
    proj: [(name, octave)] per last-frame point; points (MP_DTYPE), pdesc, local: [name] per local-map point)."""
    rng = np.random.default_rng(20240)
    lv = tc.Levels()
    cur_k, cur_d = [], []
    last_k, last_d, xw, proj = [], [], [], []
    pts, pdesc, local = [], [], []

    def member(x, y, desc, octave=0):
        cur_k.append(_kp(x, y, octave)); cur_d.append(np.asarray(desc, np.uint8))
        return len(cur_k) - 1

    def last_point(name, u, v, desc, octave=0):
        last_k.append(_kp(u, v, octave)); last_d.append(np.asarray(desc, np.uint8)); xw.append(point_at(u, v)); proj.append((name, octave))

    def local_point(name, u, v, desc):
        X = point_at(u, v).astype(np.float64); dist = np.linalg.norm(X)
        r = np.zeros((), fc.MP_DTYPE)
        r["xw"] = X; r["normal"] = X / dist                        # seen head-on: viewCos = 1 > 0.998, the radius factor is 2.5
        r["max_distance"] = dist * 1.2 ** -0.5                     # PredictScale = ceil(-0.5) = level 0
        r["min_distance"] = r["max_distance"] / float(lv.scale[-1])
        r["flags"] = 3
        pts.append(r); pdesc.append(np.asarray(desc, np.uint8)); local.append(name)

    # dense windows of 16, 17, 64 and 65 members, all of them hits for both matchers (radius 20, members within 14 px, octave 0)
    for n, u in DENSE:
        v = 403.0
        base = fc.rand_desc(rng)
        x = u + rng.uniform(-14, 14, n); y = v + rng.uniform(-14, 14, n)
        first = len(cur_k)
        probe = np.array([_kp(a, b, 0) for a, b in zip(x, y)], KP_DTYPE)
        px, py = cells(probe)
        rank = np.empty(n, np.int64); rank[np.lexsort((np.arange(n), px * ROWS + py))] = np.arange(n)
        for j in range(n):
            member(x[j], y[j], _prefix(base, n - 1 - rank[j]))
        assert len(cur_k) == first + n
        last_point("distinct_%d" % n, u, v, base); last_point("tied_%d" % n, u, v, _alternate(base))
        if n >= 64:
            local_point("distinct_%d" % n, u, v, base); local_point("tied_%d" % n, u, v, _alternate(base))
    # windows of exactly 16 and 17 grid columns (radius 20 * scale[7] = 71.66): members in the first and in the last column of the
    # walk lie outside the radius, the others are hits
    for name, u in (("span_16", 325.0), ("span_17", 121.0)):
        v = 85.0
        base = fc.rand_desc(rng)
        for dx, bits in ((-78.0, 3), (-60.0, 20), (-20.0, 7), (10.0, 7), (55.0, 31), (79.0, 2)):
            member(u + dx, v + rng.uniform(-30, 30), fc.flipped(base, bits, rng), octave=7)
        last_point(name, u, v, base, octave=7)
    # a window cut by each border of the image
    for name, (u, v), (ox, oy) in (("clip_left", (8.0, 253.0), ((-6, 2, 9), (0, 4, -5))), ("clip_right", (632.0, 253.0), ((-9, -3, 2), (0, 4, -5))),
                                   ("clip_top", (563.0, 8.0), ((0, 4, -5), (-6, 2, 9))), ("clip_bottom", (563.0, 472.0), ((0, 4, -5), (-9, -3, 2)))):
        base = fc.rand_desc(rng)
        for dx, dy, bits in zip(ox, oy, (12, 5, 9)):
            member(u + dx, v + dy, fc.flipped(base, bits, rng))
        last_point(name, u, v, base)
    # the local-map search alone: a window cut at the top-left corner
    base = fc.rand_desc(rng)
    for dx, dy, bits in ((-6, -5, 9), (3, 4, 30), (9, -2, 4)):
        member(8.0 + dx, 8.0 + dy, fc.flipped(base, bits, rng))
    local_point("clip_corner", 8.0, 8.0, base)

    def frame(k, d):
        n = len(k)
        return dict(kp=np.array(k, KP_DTYPE), desc=np.array(d, np.uint8).reshape(n, 32), ur=np.full(n, -1, F32), depth=np.full(n, -1, F32), Tcw=IDENTITY)

    return dict(last=frame(last_k, last_d), cur=frame(cur_k, cur_d), xw=np.array(xw, F32), flags=np.full(len(xw), 3, np.uint8), proj=proj,
                points=np.array(pts, fc.MP_DTYPE), pdesc=np.array(pdesc, np.uint8).reshape(len(pts), 32), local=local)


def proj_windows(sc, scale):
    """Per last-frame point, from the camera and the radius alone: name -> dict(walk(...), hits = the members k_proj_candidates keeps,
    in visiting order, dist = their Hamming distances)."""
    cur = sc["cur"]
    u, v = project(sc["xw"])
    out = {}
    for i, (name, octave) in enumerate(sc["proj"]):
        r = F32(TH_PROJ) * F32(scale[octave])
        w = walk(cur["kp"], u[i], v[i], r)
        k = cur["kp"][w["order"]]
        d = hamming(sc["last"]["desc"][i], cur["desc"][w["order"]])
        keep = in_radius(cur["kp"], w["order"], u[i], v[i], r) & (k["octave"] >= octave - 1) & (k["octave"] <= octave + 1) & (d <= TH_HIGH)
        w.update(hits=w["order"][keep], dist=d[keep], outside=int((~keep).sum()))
        out[name] = w
    return out


def local_windows(sc, scale):
    """Per local-map point: name -> dict(walk(...), hits = the members k_local_candidates counts, dist = their distances)."""
    cur = sc["cur"]
    u, v = project(sc["points"]["xw"])
    out = {}
    for i, name in enumerate(sc["local"]):
        r = F32(2.5) * F32(TH_LOCAL) * F32(scale[0])
        w = walk(cur["kp"], u[i], v[i], r)
        k = cur["kp"][w["order"]]
        keep = in_radius(cur["kp"], w["order"], u[i], v[i], r) & (k["octave"] <= 0)
        w.update(hits=w["order"][keep], dist=hamming(sc["pdesc"][i], cur["desc"][w["order"]])[keep])
        out[name] = w
    return out
