"""Shared by test_frame_cases.py and test_gpu_frame_cases.py: CRAFTED inputs for the stage that turns raw images into a Frame and for
the dense cloud -- k_cloud_mark / k_cloud_emit (csrc/k_cloud.h), k_grid_cells / k_grid_sort / k_unproject / k_undistort_* / k_cvt_gray /
k_depth_to_f32 / k_hamming_matrix (csrc/k_frame.h), k_cvt_gray3_wide (csrc/k_fast.h) and sd_image_bounds.  Plain numpy; nothing here
touches the GPU at import.  Every operation has a numpy restatement here (np_*), a second statement beside the oracle's
(oracle/oracle.py, oracle/cloud_oracle.py); the CPU tests hold the two equal and show that each crafted set holds the edge it claims,
the GPU tests compare the kernels with the oracle bit for bit.  A set's seed depends on its kind and parameters only.

Domain (check_domain_*): what the references assume and no test leaves -- no NaN / inf produced, the undistortion's denominators
1 + k1 r^2 + k2 r^4 + k3 r^6 above 0.1 in all five iterations, grid coordinates small enough that (int)roundf is defined, counts <= cap,
depths finite (inf is outside: 0 * inf)."""
import numpy as np

import stereo_cases as sc

KP_DTYPE = sc.KP_DTYPE
F32, F64 = np.float32, np.float64
SEED = 57
MAXB = 64
GRID_COLS, GRID_ROWS, GRID_CELLS = 64, 48, 64 * 48

# sd_frame_boxes of include/sd_frontend.h
BOXES_DTYPE = np.dtype([("nb", "<i4"), ("n_all", "<i4"), ("n_static", "<i4"), ("n_dynamic", "<i4"), ("boxes", "<f8", (MAXB, 4)),
                        ("box_idx", "<i4", (MAXB,)), ("box_status", "<i4", (MAXB,)), ("kept_orig", "<i4", (MAXB,)),
                        ("box_start", "<i4", (MAXB + 1,)), ("pad_", "<i4")])
CLOUD_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])

GEOM = sc.GEOMS["752x240-8x1.2"]                  # the workspace of the key-point tests (grid, unproject, undistortion)
# cols3 = 251: a ragged last word.  words = 7: a second pass of four waves with one idle.  rows3 = 336 > 256: the row-offset loop runs.
CLOUD_GEOMS = ("752x240-8x1.2", "1241x376-8x1.2", "1280x1008-5x2.0")
# Examples/RGB-D/TUM1.yaml
TUM1_K4 = np.array([517.306408, 516.469215, 318.643040, 255.313989], F32)
TUM1_D5 = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], F32)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def bits(a):
    """The bit patterns of a float array (u32 / u64), of a record array its bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return np.frombuffer(a.tobytes(), np.uint8)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def pose(k):
    """A non-trivial f64 Twc: rotation about a skew axis (Rodrigues) plus a translation, different for every k."""
    ax = np.array([0.3 + 0.1 * k, -0.5, 0.8 - 0.05 * k]); ax /= np.linalg.norm(ax)
    a = 0.2 + 0.15 * k
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = [0.5 * k - 0.3, -0.25 + 0.1 * k, 1.5 + k]
    return T


def padded(images, stride, pitch, fill, tail=0):
    """images (n, H, rowlen) -> flat (n * pitch + tail) array of the same dtype: row y of image i at i * pitch + y * stride, every
    other element from `fill` (a value, or a callable size -> array)."""
    images = np.asarray(images)
    n, H, L = images.shape
    assert stride >= L and pitch >= stride * H
    size = n * pitch + tail
    out = fill(size).astype(images.dtype) if callable(fill) else np.full(size, fill, images.dtype)
    for i in range(n):
        v = out[i * pitch:i * pitch + stride * H].reshape(H, stride)
        v[:, :L] = images[i]
    return out


# =====================================================================================================================================
# dense cloud
# =====================================================================================================================================
WINDOW_U16 = (0, 9, 10, 50, 51, 5000, 5001, 25000, 25001, 65535)
FACTORS = (float(F32(1.0) / F32(5000.0)), float(F32(1.0) / F32(1000.0)))
IMAGE_KINDS = ("window", "all", "none", "last", "lanes", "rows", "boxes")
SENTINEL = 0xA5


def cloud_shape(g):
    """(cols3, rows3, words, cap_points): the sampled grid of W x H and the least cap_points the ABI accepts."""
    cols3, rows3 = (g.W + 2) // 3, (g.H + 2) // 3
    return cols3, rows3, (cols3 + 63) // 64, cols3 * rows3


def cloud_camera(g):
    """fx, fy of the geometry; cx, cy fractional."""
    return dict(fx=F32(g.fx), fy=F32(g.fx * 1.01), cx=F32(g.W / 2 + 0.37), cy=F32(g.H / 2 - 0.21), mbf=F32(g.bf), mb=F32(g.bf / g.fx),
                mnMinX=F32(0), mnMaxX=F32(g.W), mnMinY=F32(0), mnMaxY=F32(g.H))


def cloud_image(g, kind, seed=0):
    """(color (H, W, 3) u8, depth (H, W) u16, mask (H, W) u8).  The sample grid (every third row / column) holds the pattern; the
    other pixels hold values that would change the result if they were read as samples.  The mask is 1 / 255 everywhere (it masks
    wherever a dynamic box lies) except in `boxes`, which has zeros inside the dynamic boxes."""
    W, H = g.W, g.H
    cols3, rows3, _, _ = cloud_shape(g)
    rng = _rng(1, IMAGE_KINDS.index(kind), W, H, seed)
    color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask = np.where((ii + jj) % 2 == 1, 1, 255).astype(np.uint8)
    r, j = np.meshgrid(np.arange(rows3), np.arange(cols3), indexing="ij")
    win = np.array(WINDOW_U16, np.uint16)
    if kind == "window":
        depth = win[(3 * ii + jj) % 10]                                   # samples: (9 r + 3 j) % 10 takes every value; so do the others
        s = None
    else:
        depth = np.full((H, W), 0 if kind in ("all", "rows", "boxes") else 1000, np.uint16)      # off the sample grid: the opposite decision
        if kind == "boxes":
            depth = win[rng.integers(0, 10, (H, W))]
        s = {"all": np.full((rows3, cols3), 1000), "none": np.zeros((rows3, cols3)), "last": np.zeros((rows3, cols3)),
             "lanes": np.where(((j == 63) & (r % 3 != 1)) | ((j == 64) & (r % 3 != 0)), 1000, 0),
             "rows": np.where(r % 5 == 2, 0, 1000), "boxes": np.full((rows3, cols3), 1000)}[kind].astype(np.uint16)
        if kind == "last":
            s[-1, -1] = 1000
        if kind == "rows":
            s[-1, :] = 1000                                                # the last row full: its offset is the sum of every row above
        depth[::3, ::3] = s
    if kind == "boxes":
        mask[36:48, 36:48] = 0                                             # inside the first box of the `edges` set: kept
        mask[66:84, 234:252] = 0                                           # inside both overlapping boxes: kept
        depth[30:60, 200:230] = 0                                          # masked AND out of the window: counts in masked_num
    return color, np.ascontiguousarray(depth), mask


def box_set(g, kind):
    """(boxes (k, 4) f64 x, y, w, h, box_status (k,))."""
    W, H = float(g.W), float(g.H)
    if kind == "none":
        b, s = [], []
    elif kind == "static":                                                # boxes everywhere, none of them dynamic
        b, s = [(0, 0, W, H), (-5, -5, W + 10, H + 10), (10, 10, 100, 100)], [1, -1, 1]
    elif kind == "decoy":                                                 # a slot the call does not name: would mask everything
        b, s = [(-5, -5, W + 10, H + 10)], [2]
    elif kind == "edges":
        b = [(30, 30, 30, 30), (90.5, 90.5, 30, 30), (150, 30, 0, 30), (-10, 150, 25, 20), (W - 20, H - 20, 100, 100),
             (200, 30, 60, 60), (230, 60, 60, 60), (300, 30, 60, 60), (400, 30, 60, 60), (500, 30, 60, 0), (560.25, 29.75, 29.5, 30.5)]
        s = [2, 0, 2, 0, 2, 2, 0, 1, -1, 2, 0]
    elif kind == "last_of_64":
        b = [(100, 100, 200, 100)] * 63 + [(150, 120, 90, 60)]
        s = [1, -1] * 31 + [1] + [2]
    else:
        raise KeyError(kind)
    return np.asarray(b, F64).reshape(-1, 4), np.asarray(s, np.int32)


def boxes_record(boxes, status):
    r = np.zeros((), BOXES_DTYPE)
    n = len(status)
    r["nb"] = n; r["boxes"][:n] = boxes; r["box_status"][:n] = status; r["box_status"][n:] = 2; r["box_idx"][:n] = 100 + np.arange(n)
    r["boxes"][n:] = (-5, -5, 1e4, 1e4)                                   # beyond nb: a dynamic box over everything, never to be read
    return r


def cloud_calls(g):
    """The launches of one geometry: dict(name, factor, use_mask, slots (three, out of order, one twice), images (a kind per frame),
    boxsets (a kind per slot of the workspace; slots 1 and 3 are not named by the call))."""
    out = []
    for fi, f in enumerate(FACTORS):
        out.append(dict(name="window-f%d" % fi, factor=f, use_mask=True, slots=[2, 0, 2], images=["window", "all", "lanes"],
                        boxsets={0: "static", 1: "decoy", 2: "none", 3: "decoy"}))
    out.append(dict(name="patterns", factor=FACTORS[1], use_mask=True, slots=[2, 0, 2], images=["none", "last", "rows"],
                    boxsets={0: "none", 1: "decoy", 2: "static", 3: "decoy"}))
    out.append(dict(name="boxes-mask", factor=FACTORS[0], use_mask=True, slots=[2, 0, 2], images=["boxes", "boxes", "window"],
                    boxsets={0: "last_of_64", 1: "decoy", 2: "edges", 3: "decoy"}))
    out.append(dict(name="boxes-nomask", factor=FACTORS[1], use_mask=False, slots=[2, 0, 2], images=["boxes", "boxes", "window"],
                    boxsets={0: "last_of_64", 1: "decoy", 2: "edges", 3: "decoy"}))
    return out


def cloud_frames(g, call):
    """Per frame of the call: dict(color, depth, mask, boxes, status, Twc)."""
    out = []
    for f, (slot, kind) in enumerate(zip(call["slots"], call["images"])):
        color, depth, mask = cloud_image(g, kind, f)
        boxes, status = box_set(g, call["boxsets"][slot])
        out.append(dict(color=color, depth=depth, mask=mask, boxes=boxes, status=status, Twc=pose(f + 1)))
    return out


def check_domain_cloud(g, fr, factor):
    assert fr["depth"].dtype == np.uint16 and fr["depth"].shape == (g.H, g.W) == fr["mask"].shape and fr["color"].shape == (g.H, g.W, 3)
    assert len(fr["status"]) == len(fr["boxes"]) <= MAXB and np.isfinite(fr["boxes"]).all() and np.isfinite(fr["Twc"]).all()
    assert np.isfinite(F32(65535) * F32(factor))
    return fr


def np_cloud(color, depth, factor, mask, boxes, status, cam, Twc, detail=False):
    """PointCloudMapping::generatePointCloud behind the dyn_boxes filter, row by row.  -> (points, masked_num[, keep, skip, d])."""
    H, W = depth.shape
    dyn = [tuple(b) for b, s in zip(np.asarray(boxes, F64).reshape(-1, 4), status) if s == 0 or s == 2]
    n = np.arange(0, W, 3)
    nf = n.astype(F32)
    T = np.asarray(Twc, F64).reshape(4, 4)
    fx, fy, cx, cy = (F32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    parts, keeps, skips, ds = [], [], [], []
    masked = 0
    for m in range(0, H, 3):
        d = depth[m, n].astype(F32) * F32(factor)
        skip = np.zeros(len(n), bool)
        if mask is not None:
            for (x, y, w, h) in dyn:
                if y <= F64(F32(m)) and F64(F32(m)) < y + h:
                    skip |= (x <= nf.astype(F64)) & (nf.astype(F64) < x + w)
            skip &= mask[m, n] != 0
        masked += int(skip.sum())
        keep = ~skip & ~(d.astype(F64) < 0.01) & ~(d > F32(5.0))
        keeps.append(keep); skips.append(skip); ds.append(d)
        z = d[keep]
        x = (nf[keep] - cx) * z; x = x / fx
        y = (F32(m) - cy) * z; y = y / fy
        p = np.zeros(len(z), CLOUD_POINT_DTYPE)
        xd, yd, zd = x.astype(F64), y.astype(F64), z.astype(F64)
        for k, name in enumerate("xyz"):
            t = T[k, 0] * xd + T[k, 1] * yd; t = t + T[k, 2] * zd; t = t + T[k, 3]
            p[name] = t.astype(F32)
        c = color[m, n[keep]]
        p["b"], p["g"], p["r"], p["a"] = c[:, 0], c[:, 1], c[:, 2], 255
        parts.append(p)
    pts = np.concatenate(parts)
    assert np.isfinite(pts["x"]).all() and np.isfinite(pts["y"]).all() and np.isfinite(pts["z"]).all()
    return (pts, masked, np.array(keeps), np.array(skips), np.array(ds)) if detail else (pts, masked)


def oracle_cloud(CO, fr, factor, use_mask, cam):
    return CO.generate_point_cloud(fr["color"], fr["depth"], factor, fr["mask"] if use_mask else None, CO.dyn_boxes(fr["boxes"], fr["status"]),
                                   cam["fx"], cam["fy"], cam["cx"], cam["cy"], fr["Twc"])


# =====================================================================================================================================
# grid
# =====================================================================================================================================
GRID_K4 = np.array([500.0, 500.0, 256.0, 192.0], F32)
GRID_D5 = np.array([0.05, -0.02, 0.001, -0.001, 0.005], F32)
GRID_ORIGINS = ((0.0, 0.0), (-13.5, -7.25))            # a distorted camera's bounds start off zero
HEAVY_CELL = 1000
SEAM_CELLS = (0, 11, 12, 767, 768, 3071)               # 12 cells per thread, 64 threads per wave


def grid_camera(origin):
    """Bounds with extents 512 x 384: the inverse cell sizes are exactly 1 / 8."""
    x0, y0 = origin
    return dict(fx=GRID_K4[0], fy=GRID_K4[1], cx=GRID_K4[2], cy=GRID_K4[3], mbf=F32(40.0), mb=F32(40.0 / 500.0), mnMinX=F32(x0),
                mnMaxX=F32(x0 + 512.0), mnMinY=F32(y0), mnMaxY=F32(y0 + 384.0))


def cam10(cam):
    return np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")], F32)


def frame_kps(x, y, seed=0):
    """Key points at (x, y) whose other fields all differ from each other and from record to record."""
    k = sc.kps(GEOM, x, y, 0)
    n = len(k)
    i = np.arange(n)
    k["octave"] = (i + seed) % GEOM.n_levels
    k["size"] = F32(31.0) * GEOM.scale[k["octave"]]
    k["angle"] = ((i * 37 + seed) % 3600).astype(F32) / F32(10.0)
    k["response"] = (20 + (i * 13 + seed) % 200).astype(F32) + F32(0.5)
    k["class_id"] = -1
    return k


def at_cell(origin, px, py):
    """The centre of cell (px, py) in image coordinates (exact in f32 for both origins)."""
    return F32(origin[0] + 8.0 * np.asarray(px, F64)), F32(origin[1] + 8.0 * np.asarray(py, F64))


HALF_POS = (-0.5, 0.5, 1.5, 31.5, 62.5, 63.5)          # exact halves of a cell, first and last included


def grid_edges(origin):
    """Grid positions (in cells) on the decisions of PosInGrid: exact halves; -0.4 -> 0 and -0.5 -> -1; the last f32 below 0.5; the far
    border and just inside it.  Every x edge against y = cell 5's centre and every y edge against x = cell 7's centre, then the
    halves against each other.  -> (kp, pos (n, 2) f64: the intended grid position)"""
    f = lambda v: float(F32(v))
    edge = list(HALF_POS) + [-0.4, f(np.nextafter(F32(-0.5), F32(0))), f(np.nextafter(F32(0.5), F32(0))), f(np.nextafter(F32(63.5), F32(0))),
                             63.0, 63.4375, 64.0, -0.0625, 0.0]
    P = [(e, 5.0) for e in edge] + [(7.0, e) for e in edge if e < GRID_ROWS + 1] + [(47.5, 47.5), (46.5, 47.4375), (7.0, 47.5), (7.0, 48.0), (7.0, 46.5)]
    P += [(a, b) for a in HALF_POS for b in (-0.5, 0.5, 31.5, 46.5, 47.5)]
    pos = np.array(P, F64)
    x = F32(origin[0]) + (pos[:, 0] * 8.0).astype(F32); y = F32(origin[1]) + (pos[:, 1] * 8.0).astype(F32)
    return frame_kps(x, y, 1), pos


def grid_random(origin, n, seed, frac_out=0.1):
    """n key points over the grid and a margin around it (about frac_out of them outside), in random index order."""
    rng = _rng(2, n, seed)
    m = 512 * frac_out / 4
    x = rng.uniform(origin[0] - 4 - m, origin[0] + 508 + m, n); y = rng.uniform(origin[1] - 4 - m, origin[1] + 380 + m, n)
    return frame_kps(x, y, seed)


def grid_all_out(origin, n=300):
    rng = _rng(3, n)
    side = rng.integers(0, 4, n)
    x = np.where(side == 0, origin[0] - rng.uniform(4.5, 200, n), np.where(side == 1, origin[0] + 508 + rng.uniform(0.5, 200, n), rng.uniform(origin[0], origin[0] + 500, n)))
    y = np.where(side == 2, origin[1] - rng.uniform(4.5, 200, n), np.where(side == 3, origin[1] + 380 + rng.uniform(0.5, 200, n), rng.uniform(origin[1], origin[1] + 370, n)))
    return frame_kps(x, y, 3)


def grid_one_cell(origin, n, cell=HEAVY_CELL, seed=4):
    rng = _rng(4, n, cell)
    cx, cy = at_cell(origin, cell // GRID_ROWS, cell % GRID_ROWS)
    return frame_kps(cx + rng.uniform(-3.9, 3.9, n), cy + rng.uniform(-3.9, 3.9, n), seed)


def grid_heavy(origin):
    """300 members in HEAVY_CELL and one in each of SEAM_CELLS, the singles spread among the members' indices (index order is not
    cell order: the singles of the high cells come first)."""
    k = grid_one_cell(origin, 300 + len(SEAM_CELLS))
    for i, c in enumerate(reversed(SEAM_CELLS)):
        k["x"][40 * i + 3], k["y"][40 * i + 3] = at_cell(origin, c // GRID_ROWS, c % GRID_ROWS)
    return k


GRID_COUNTS = (0, 1, 255, 256, 257)


def grid_sets(origin, cap):
    """[(name, kp)]: every crafted frame of one camera."""
    out = [("edges", grid_edges(origin)[0]), ("all_out", grid_all_out(origin)), ("one_cell", grid_one_cell(origin, 600)), ("heavy", grid_heavy(origin)),
           ("one_cell_cap", grid_one_cell(origin, cap, 1535, 5))]
    out += [("count%d" % n, grid_random(origin, n, n)) for n in GRID_COUNTS + (cap,)]
    return out


def c_roundf(v):
    """C roundf of f32 values (halves away from zero), exact: v +- 0.5 is formed in f64."""
    v = np.asarray(v, F32).astype(F64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def np_grid_cells(kp, cam):
    """Frame::PosInGrid: round((x - mnMinX) * mfGridElementWidthInv), products and differences in f32.  -> cell id or -1 (i32)"""
    wInv = F32(GRID_COLS) / (F32(cam["mnMaxX"]) - F32(cam["mnMinX"])); hInv = F32(GRID_ROWS) / (F32(cam["mnMaxY"]) - F32(cam["mnMinY"]))
    px = c_roundf((kp["x"] - F32(cam["mnMinX"])) * wInv); py = c_roundf((kp["y"] - F32(cam["mnMinY"])) * hInv)
    ok = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    return np.where(ok, px * GRID_ROWS + py, -1).astype(np.int32)


def np_grid_index(cell):
    """(sortedIdx, cellStart[3073]): the in-grid key points' indices in a STABLE sort by cell id (mGrid's push_back order inside a cell);
    cellStart[c] = the number of in-grid key points in cells below c."""
    cell = np.asarray(cell, np.int64)
    idx = np.nonzero(cell >= 0)[0]
    idx = idx[np.argsort(cell[idx], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(cell[cell >= 0], minlength=GRID_CELLS))])
    return idx.astype(np.uint16), start.astype(np.uint16)


def check_domain_kp(kp, cam, cap, dist=None):
    """(int)roundf is defined (|grid position| far below 2^31), count <= cap <= 65535, finite coordinates; with a distortion its
    denominators stay above 0.1."""
    assert kp.dtype == KP_DTYPE and len(kp) <= cap <= 65535
    assert np.isfinite(kp["x"]).all() and np.isfinite(kp["y"]).all()
    assert (np.abs(kp["x"]) < 1e5).all() and (np.abs(kp["y"]) < 1e5).all()
    if dist is not None:
        check_domain_undistort(np.stack([kp["x"], kp["y"]], 1), dist[0], dist[1])
    return kp


# =====================================================================================================================================
# undistortion and bounds
# =====================================================================================================================================
def np_undistort(pts, K4, dist5, iters=5, denominators=False):
    """cv::undistortPoints(pts, K, dist, Mat(), K): `iters` fixed-point iterations in f64, narrowed to f32."""
    p = np.asarray(pts, F32).reshape(-1, 2).astype(F64)
    fx, fy, cx, cy = (F64(v) for v in np.asarray(K4, F32))
    k1, k2, p1, p2, k3 = (F64(v) for v in np.asarray(dist5, F32))
    ifx, ify = 1.0 / fx, 1.0 / fy
    x = (p[:, 0] - cx) * ifx; y = (p[:, 1] - cy) * ify
    x0, y0 = x, y
    den = []
    for _ in range(iters):
        r2 = x * x + y * y
        dn = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        den.append(dn)
        icdist = 1.0 / dn
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist
    out = np.stack([(x * fx + cx).astype(F32), (y * fy + cy).astype(F32)], 1)
    return (out, np.array(den)) if denominators else out


def check_domain_undistort(pts, K4, dist5):
    out, den = np_undistort(pts, K4, dist5, denominators=True)
    assert np.isfinite(out).all(), "undistortion produced a NaN or inf"
    assert den.size == 0 or den.min() > 0.1, "undistortion denominator %g" % den.min()
    return out


def np_image_bounds(cols, rows, K4, dist5):
    if np.asarray(dist5, F32)[0] == 0:
        return np.array([0, cols, 0, rows], F32)
    u = np_undistort([[0, 0], [cols, 0], [0, rows], [cols, rows]], K4, dist5)
    return np.array([min(u[0, 0], u[2, 0]), max(u[1, 0], u[3, 0]), min(u[0, 1], u[1, 1]), max(u[2, 1], u[3, 1])], F32)


UN_W, UN_H = 640, 480
# each coefficient alone: TUM1's where the iteration converges on points 50 px outside the image; k2 and k3 alone are taken smaller
# (TUM1's k2 = -0.95 without its k1 and k3 drives the denominator through zero there)
SINGLE_D5 = np.array([0.262383, -0.05, -0.005358, 0.002628, 0.3], F32)
IDENTITY_RULE_D5 =np.array([0.0, 0.1, 0.01, 0.01, 0.1], F32)       # k1 == 0: mvKeysUn = mvKeys whatever the others are


def coefficient_sets():
    """[(name, dist5)]: each coefficient alone, TUM1's set, the k1 == 0 rule's set."""
    out = []
    for i, name in enumerate(("k1", "k2", "p1", "p2", "k3")):
        d = np.zeros(5, F32); d[i] = SINGLE_D5[i]
        out.append((name, d))
    return out + [("tum1", TUM1_D5.copy()), ("k1_zero", IDENTITY_RULE_D5.copy())]


def undistort_points():
    """(pts (n, 2) f32, names of the first entries): the corners, 50 px outside each side, the principal point, then random points in
    and around the image (n = 300, so that n in {0, 1, 255, 256, 257} are prefixes)."""
    W, H = float(UN_W), float(UN_H)
    named = [("corner00", (0, 0)), ("corner10", (W, 0)), ("corner01", (0, H)), ("corner11", (W, H)), ("left", (-50, H / 2)), ("right", (W + 50, H / 2)),
             ("top", (W / 2, -50)), ("bottom", (W / 2, H + 50)), ("principal", (TUM1_K4[2], TUM1_K4[3])), ("out00", (-50, -50)), ("out11", (W + 50, H + 50))]
    rng = _rng(6)
    rnd = np.stack([rng.uniform(-50, W + 50, 300 - len(named)), rng.uniform(-50, H + 50, 300 - len(named))], 1)
    return np.concatenate([np.array([p for _, p in named], F32), rnd.astype(F32)]), [n for n, _ in named]


UN_COUNTS = (0, 1, 255, 256, 257)


# =====================================================================================================================================
# UnprojectStereo
# =====================================================================================================================================
EDGE_DEPTHS = np.array([0.0, -1.0, -0.0, np.nan, 1e-30, 1e-38, 0.01, 80.0], F32)


def unproject_frame(n, seed, cam):
    """(kp, depth): the edge depths against key points at (cx, cy) exactly and at ordinary places, then random positive depths."""
    rng = _rng(7, n, seed)
    x = rng.uniform(0, 640, n).astype(F32); y = rng.uniform(0, 480, n).astype(F32)
    d = rng.uniform(0.3, 40.0, n).astype(F32)
    e = len(EDGE_DEPTHS)
    m = min(n, 3 * e)
    d[:m] = np.tile(EDGE_DEPTHS, 3)[:m]
    x[:min(n, e)] = cam["cx"]; y[:min(n, e)] = cam["cy"]                    # every edge depth once at the principal point
    if n > 3 * e + 2:
        x[3 * e] = cam["cx"]; y[3 * e + 1] = cam["cy"]                      # and one coordinate each on it at an ordinary depth
    return frame_kps(x, y, seed), d


def np_unproject(kp, depth, cam, Twc):
    """Frame::UnprojectStereo in f32, left to right: x3Dc = ((u - cx) * z * invfx, (v - cy) * z * invfy, z); Rwc * x3Dc + Ow."""
    T = np.asarray(Twc, F32).reshape(4, 4)
    z = np.asarray(depth, F32)
    ok = z > 0
    invfx, invfy = F32(1.0) / F32(cam["fx"]), F32(1.0) / F32(cam["fy"])
    with np.errstate(all="ignore"):
        x = (kp["x"] - F32(cam["cx"])) * z * invfx; y = (kp["y"] - F32(cam["cy"])) * z * invfy
        xw = np.zeros((len(z), 3), F32)
        for k in range(3):
            s = T[k, 0] * x + T[k, 1] * y; s = s + T[k, 2] * z; xw[:, k] = s + T[k, 3]
    xw[~ok] = 0
    assert np.isfinite(xw).all()
    return xw, ok.astype(np.uint8)


def check_domain_depth(d):
    assert not np.isinf(d).any(), "inf depth is outside the domain"
    return d


# =====================================================================================================================================
# cvtColor, depth conversion, Hamming
# =====================================================================================================================================
CVT_WIDTHS = (1, 3, 4, 5, 15, 16, 17, 31, 33, 1023, 1024, 1025)       # 16 pixels per thread in the wide kernel, 4 in the other
CVT_HEIGHTS = (1, 3, 4, 5)
DEPTH_FACTORS = (FACTORS[0], FACTORS[1], float(F32(1.0) / F32(5208.0)), 1.0)
DEPTH_WIDTHS, DEPTH_HEIGHTS = (1, 63, 64, 65), (1, 3, 5)
HAMMING_SIZES = (1, 3, 4, 5, 63, 64, 65)


def np_cvt_gray(img, rgb_order):
    """cv::cvtColor(RGB|BGR[A]2GRAY) on 8 bits: (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14; a 4th channel is ignored."""
    p = np.asarray(img, np.uint8).astype(np.int32)
    r, b = (p[..., 0], p[..., 2]) if rgb_order else (p[..., 2], p[..., 0])
    return ((r * 4899 + p[..., 1] * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def all_triples(channels, seed=0):
    """(4096, 4096, channels) u8: every (c0, c1, c2) once; a 4th channel is random."""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    out = np.empty((4096, 4096, channels), np.uint8)
    out[..., 0] = i & 255; out[..., 1] = (i >> 8) & 255; out[..., 2] = i >> 16
    if channels == 4:
        out[..., 3] = _rng(8, seed).integers(0, 256, (4096, 4096), dtype=np.uint8)
    return out


def cvt_images(w, h, channels, seed=0, n=3):
    return _rng(9, w, h, channels, seed).integers(0, 256, (n, h, w, channels), dtype=np.uint8)


def np_depth_to_f32(d, factor):
    return np.asarray(d, np.uint16).astype(F32) * F32(factor)


def all_u16():
    return np.arange(65536, dtype=np.uint16).reshape(256, 256)


def np_hamming(a, b):
    return np.unpackbits(np.asarray(a, np.uint8)[:, None, :] ^ np.asarray(b, np.uint8)[None, :, :], axis=2).sum(axis=2).astype(np.uint16)


def hamming_sets():
    """[(a (na, 32), b (nb, 32), planted)]: for every (na, nb) of HAMMING_SIZES, b[j] = a[j % na] with planted[j] bits inverted; the
    planted distances run on from set to set, so together they take every value 0 .. 256."""
    out, c = [], 0
    for na in HAMMING_SIZES:
        for nb in HAMMING_SIZES:
            rng = _rng(10, na, nb)
            a = sc.rand_desc(rng, na)
            planted = (c + np.arange(nb)) % 257
            b = sc.flipped(rng, a[np.arange(nb) % na], planted)
            out.append((a, b, planted))
            c += nb
    return out


# =====================================================================================================================================
# the device side (tests marked gpu)
# =====================================================================================================================================
class Workspace:
    """n_slots image slots of one geometry, made valid by ONE extraction of blank images; the tests then write key points, counts,
    depths, map points and box records straight into the slots' device arrays."""

    def __init__(self, fe, g, n_slots=4):
        import ctypes as C
        import torch
        self.fe, self.g, self.n = fe, g, n_slots
        self.ex = fe.ORBextractor(*g.extractor_args())
        self.b = fe.Batch(self.ex, g.W, g.H, n_slots)
        kp_p, _, cnt_p, self.cap = self.b.results_device()
        n, cap = n_slots, self.cap
        self.kp = fe.as_torch_u8(kp_p, n * cap * KP_DTYPE.itemsize).view(n, cap * KP_DTYPE.itemsize)
        self.count = fe.as_torch_u8(cnt_p, n * 4).view(torch.int32)
        _, dep_p, _ = self.b.stereo_device()
        self.depth = fe.as_torch_u8(dep_p, n * cap * 4).view(torch.float32).view(n, cap)
        xw_p, fl_p, c = C.c_void_p(), C.c_void_p(), C.c_int()
        fe.check(fe.lib().sd_batch_mappoints_device(self.b.h, C.byref(xw_p), C.byref(fl_p), C.byref(c)))
        self.xw = fe.as_torch_u8(xw_p.value, n * cap * 12).view(torch.float32).view(n, cap, 3)
        self.flags = fe.as_torch_u8(fl_p.value, n * cap).view(n, cap)
        assert BOXES_DTYPE.itemsize == fe.FRAME_BOXES_BYTES
        self.boxes = fe.as_torch_u8(fe.batch_boxes_device(self.b), n * fe.FRAME_BOXES_BYTES).view(n, fe.FRAME_BOXES_BYTES)
        self.b.extract_host(np.full((n, g.H, g.W), 128, np.uint8))
        self.b.sync()
        self.set_boxes({s: boxes_record(*box_set(g, "none")) for s in range(n)})

    def close(self):
        self.b.close()

    def set_boxes(self, records):
        import torch
        for s, r in records.items():
            self.boxes[s] = torch.from_numpy(np.frombuffer(r.tobytes(), np.uint8).copy()).cuda()
        torch.cuda.synchronize()

    def set_kps(self, frames):
        """frames: {slot: kp}: key points and count of the slot."""
        import torch
        for s, k in frames.items():
            assert len(k) <= self.cap
            if len(k):
                self.kp[s, :k.nbytes] = torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda()
            self.count[s] = len(k)
        torch.cuda.synchronize()

    def set_depth(self, depths):
        import torch
        for s, d in depths.items():
            self.depth[s, :len(d)] = torch.from_numpy(np.ascontiguousarray(d, F32)).cuda()
        torch.cuda.synchronize()


def run_cloud(ws, call, cap_points=None, fill=SENTINEL, stream=None):
    """One sd_batch_backproject_dense on the call's three frames: colour, depth and mask with padded strides and pitches (depth and
    mask strides differ; the padding holds depths that would be kept and mask values that would mask).  stream: a HIP stream handle to
    launch on (the inputs are complete before the call).
    -> (counts (n, 2) i32, points (n, cap_points) CLOUD_POINT_DTYPE, frames, the SdError of a refused call or None)"""
    import torch
    g = ws.g
    W, H = g.W, g.H
    frames = [check_domain_cloud(g, fr, call["factor"]) for fr in cloud_frames(g, call)]
    n = len(frames)
    cap_points = cloud_shape(g)[3] if cap_points is None else cap_points
    ws.set_boxes({s: boxes_record(*box_set(g, k)) for s, k in call["boxsets"].items()})
    rng = _rng(11, W, H)
    cs, ds, ms = 3 * W + 7, W + 5, W + 9
    cp, dp, mp = cs * H + 13, ds * H + 3, ms * H + 11
    color = padded(np.stack([f["color"].reshape(H, 3 * W) for f in frames]), cs, cp, lambda k: rng.integers(0, 256, k))
    depth = padded(np.stack([f["depth"] for f in frames]), ds, dp, 1000)
    mask = padded(np.stack([f["mask"] for f in frames]), ms, mp, 255)
    d_color = torch.from_numpy(color).cuda(); d_depth = torch.from_numpy(depth.view(np.int16)).cuda(); d_mask = torch.from_numpy(mask).cuda()
    d_pts = torch.full((n, cap_points, CLOUD_POINT_DTYPE.itemsize), fill, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    err = None
    torch.cuda.synchronize()
    try:
        ws.b.backproject_dense(call["slots"], d_color.data_ptr(), cs, cp, d_depth.data_ptr(), ds, dp, call["factor"],
                               d_mask.data_ptr() if call["use_mask"] else 0, ms, mp, cloud_camera(g), np.stack([f["Twc"] for f in frames]),
                               d_pts.data_ptr(), cap_points, d_cnt.data_ptr(), stream=stream)
    except ws.fe.SdError as e:
        err = e
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy(); pts = d_pts.cpu().numpy().reshape(n, -1).view(CLOUD_POINT_DTYPE)
    return cnt, pts, frames, err
