"""Shared by test_oracle_motion.py, test_gpu_motion.py and tools/fuzz_motion.py: seeded point-pair sets for the TrackHomo model
fit (spec Q13).  Plain numpy; every generator returns (p1, p2) = (points_last, points_current) as (N, 2) f32.  A set's seed
depends on its kind and size only, never on its place in a list, so the CPU tests that say which branch a set reaches and
the GPU tests that run it speak of the same points."""
import numpy as np

SEED = 20
W, H = 1241.0, 376.0                                          # the KITTI image the scenes are drawn in
SIZES = (0, 1, 7, 8, 9, 10, 11, 12, 19, 20, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 2047, 2048, 2049, 4095, 4096, 4097)
DEGENERATE_KINDS = ("same_x1", "same_y1", "same_x2", "same_y2", "all_equal", "collinear", "three_distinct")
KINDS = (("planar", 0.0), ("planar", 0.30), ("planar", 0.55), ("general", 0.20), ("general", 0.45), ("noise_only", None))
HT = np.array([[1.02, 0.01, 6.0], [-0.005, 1.02, -3.0], [1e-5, -2e-5, 1.0]])
K = np.array([[707.0, 0, 601.9], [0, 707.0, 183.1], [0, 0, 1]])


def _uniform(rng, n):
    return np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)


def _f32(p1, p2):
    return np.ascontiguousarray(p1, np.float32).reshape(-1, 2), np.ascontiguousarray(p2, np.float32).reshape(-1, 2)


def _with_outliers(rng, p2, outlier_frac):
    out = rng.random(len(p2)) < outlier_frac
    p2[out] = _uniform(rng, int(out.sum()))
    return p2


def planar(rng, N, outlier_frac, noise):
    """One homography (a 2 % zoom, a small rotation and perspective, a shift) + Gaussian noise; an outlier_frac share of p2 is
    replaced by unrelated points."""
    p1 = _uniform(rng, N).astype(np.float32)
    q = (HT @ np.c_[p1, np.ones(N)].T).T
    p2 = q[:, :2] / q[:, 2:] + rng.normal(0, noise, (N, 2))
    return _f32(p1, _with_outliers(rng, p2, outlier_frac))


def general(rng, N, outlier_frac, noise):
    """Points 4 - 40 m deep under a sideways translation: no single homography explains them, a fundamental matrix does."""
    X = np.stack([rng.uniform(-8, 8, N), rng.uniform(-2, 2, N), rng.uniform(4, 40, N)], 1)
    p1 = (K @ X.T).T; p1 = p1[:, :2] / p1[:, 2:]
    p2 = (K @ (X + np.array([0.9, 0.05, -0.3])).T).T; p2 = p2[:, :2] / p2[:, 2:] + rng.normal(0, noise, (N, 2))
    return _f32(p1, _with_outliers(rng, p2, outlier_frac))


def noise_only(rng, N):
    return _f32(_uniform(rng, N), _uniform(rng, N))


def degenerate(kind, N):
    """same_*: a planar scene with one of the four coordinates constant (zero spread: no normalisation).  all_equal: one point
    pair N times.  three_distinct: three point pairs in turn (every 4- and 8-sample repeats a pair: all systems singular).
    collinear: points of one line under a translation -- every 4-point system is singular or close to it, yet the fit exists."""
    rng = np.random.default_rng([SEED, 7, DEGENERATE_KINDS.index(kind), N])
    p1, p2 = planar(rng, N, 0.0, 0.4)
    if kind.startswith("same_"):
        (p1 if kind[-1] == "1" else p2)[:, 0 if kind[5] == "x" else 1] = np.float32(123.5)
    elif kind == "all_equal":
        p1[:] = np.float32([10.0, 20.0]); p2[:] = np.float32([10.0, 20.0])
    elif kind == "three_distinct":
        a = np.float32([[100, 50], [700, 300], [1100, 90]]); b = np.float32([[104, 48], [707, 305], [1111, 86]])
        p1 = a[np.arange(N) % 3]; p2 = b[np.arange(N) % 3]
    elif kind == "collinear":
        t = rng.uniform(0, 1, N)
        p1 = np.stack([50 + 1100 * t, 40 + 290 * t], 1); p2 = p1 + np.array([5.0, -2.0])
    else:
        raise ValueError(kind)
    return _f32(p1, p2)


def all_inliers(N):
    """Integer points under an exact integer translation.  Both normalised point sets are then the same bits, the columns of
    every eight-point system repeat each other, and every F hypothesis is degenerate: n_h == N, n_f == 0."""
    rng = np.random.default_rng([SEED, 8, N])
    p1 = np.stack([rng.integers(0, 1241, N), rng.integers(0, 376, N)], 1).astype(np.float64)
    return _f32(p1, p1 + np.array([7.0, -4.0]))


def scaled(rng, N, offset, spread):
    """Coordinates within `spread` of `offset` in both images (a planar scene squeezed into that window): far from the origin
    the f32 grid is coarse against the spread, points coincide, and the normalisation carries all the conditioning."""
    p1, p2 = planar(rng, N, 0.1, 0.4)
    s = spread / W
    return _f32(offset + p1.astype(np.float64) * s, offset + p2.astype(np.float64) * s)


def exact_share(N, n_in):
    """Exactly n_in pairs under an integer translation, the others unrelated (integer points): the best H count is n_in, which the
    caller puts one below, on and one above the checkpoint bound 0.53 N."""
    rng = np.random.default_rng([SEED, 10, N, n_in])
    p1 = np.stack([rng.integers(0, 1241, N), rng.integers(0, 376, N)], 1).astype(np.float64)
    p2 = p1 + np.array([7.0, -4.0])
    out = rng.permutation(N)[n_in:]
    p2[out] = np.stack([rng.integers(0, 1241, len(out)), rng.integers(0, 376, len(out))], 1)
    return _f32(p1, p2)


EXACT_SHARES = ((100, 52), (100, 53), (100, 54), (200, 105), (200, 106), (200, 107))
SCALED = ((-300.0, 50.0), (-1e4, 200.0), (1e4, 200.0), (1e4, 1e-2), (0.0, 1e-2), (-5.0, 1e-2))
ALL_INLIERS_SIZES = (8, 9, 10, 11, 12, 300, 2100)
DEGENERATE_SIZES = (8, 50, 300)


def make(kind, N, frac=None):
    """The set of the size x kind product: the same points whoever asks."""
    rng = np.random.default_rng([SEED, ("planar", "general", "noise_only").index(kind), int(round(100 * (frac or 0))), N])
    if kind == "planar":
        return planar(rng, N, frac, 0.4)
    if kind == "general":
        return general(rng, N, frac, 0.3)
    return noise_only(rng, N)


def suite(capacities=(), max_n=None):
    """[(name, p1, p2)]: every size (SIZES plus capacity - 1 and capacity of each workspace named) x KINDS, then the degenerate,
    all_inliers, exact_share and scaled sets; max_n drops the sets that a workspace of that capacity cannot hold."""
    sizes = sorted(set(SIZES) | {c - d for c in capacities for d in (0, 1)})
    out = []
    for N in sizes:
        for kind, frac in KINDS:
            out.append(("%s-%s-N%d" % (kind, "%d%%" % round(100 * frac) if frac is not None else "x", N),) + make(kind, N, frac))
    for N in DEGENERATE_SIZES:
        for kind in DEGENERATE_KINDS:
            out.append(("degenerate-%s-N%d" % (kind, N),) + degenerate(kind, N))
    for N in ALL_INLIERS_SIZES:
        out.append(("all_inliers-N%d" % N,) + all_inliers(N))
    for N, n_in in EXACT_SHARES:
        out.append(("exact_share-N%d-%d" % (N, n_in),) + exact_share(N, n_in))
    for j, (offset, spread) in enumerate(SCALED):
        for N in (40, 600):
            out.append(("scaled-%g-%g-N%d" % (offset, spread, N),) + scaled(np.random.default_rng([SEED, 9, j, N]), N, offset, spread))
    return [s for s in out if max_n is None or len(s[1]) <= max_n]


# ---- the device side (tests marked gpu and tools/fuzz_motion.py): point sets written over a workspace's projection pairs

class Workspace:
    """2 * n_sets extracted images of one extractor without distortion: slots 2k (Last) and 2k + 1 (Current) carry set k.  The
    slots are scratch once run_sets has been called."""

    def __init__(self, fe, synth, cfg, n_sets):
        import torch
        self.fe, self.n_sets, self.cam = fe, n_sets, fe.make_camera(cfg)
        W_, H_, n = cfg["width"], cfg["height"], 2 * n_sets
        ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
        self.b = b = fe.Batch(ex, W_, H_, n)
        img = synth.stereo_frame(seq=6, t=0, cfg=cfg)[0]
        b.extract_host(np.stack([img] * n))
        depth = torch.full((n, H_, W_), 10.0, dtype=torch.float32, device="cuda")
        b.rgbd_from_f32(depth.data_ptr(), W_, W_ * H_, n, cfg["bf"])
        b.assign_grid(n, self.cam)
        b.unproject(1, n, self.cam, np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)))
        b.sync()
        kp_p, _, _, self.cap = b.results_device()
        _, pairs_p, npairs_p, _, _ = b.matches_device()
        kp_bytes = fe.as_torch_u8(kp_p, n * self.cap * fe.KP_DTYPE.itemsize)
        self.kp0 = kp_bytes.clone()                                  # what the extractor left: restored before every search
        self.kp_bytes = kp_bytes
        self.kp = kp_bytes.view(torch.float32).view(n, self.cap, fe.KP_DTYPE.itemsize // 4)      # x, y = words 0, 1
        self.pairs = fe.as_torch_u8(pairs_p, n * self.cap * 8).view(torch.int32).view(n, self.cap, 2)
        self.npairs = fe.as_torch_u8(npairs_p, n * 4).view(torch.int32)

    def close(self):
        self.b.close()


def run_sets(ws, sets):
    """The device fit of len(sets) point sets [(p1, p2)] in one launch: one real SearchByProjection over that many pairs fixes the
    pair count and the pair -> slot table, then set k's points overwrite x, y of the key points of slots 2k / 2k + 1, its pair
    list becomes (i, i), i < N, and its pair count N."""
    import torch
    b, S = ws.b, len(sets)
    assert 0 < S <= ws.n_sets and all(len(p1) == len(p2) <= ws.cap for p1, p2 in sets)
    ws.kp_bytes.copy_(ws.kp0)
    torch.cuda.synchronize()
    I = np.tile(np.eye(4, dtype=np.float32), (S, 1, 1))
    b.search_by_projection([2 * k + 1 for k in range(S)], [2 * k for k in range(S)], I, I, ws.cam, 15.0, False, True)
    b.sync()
    for k, (p1, p2) in enumerate(sets):
        N = len(p1)
        if N:
            ws.kp[2 * k, :N, 0:2] = torch.from_numpy(np.ascontiguousarray(p1, np.float32)).cuda()
            ws.kp[2 * k + 1, :N, 0:2] = torch.from_numpy(np.ascontiguousarray(p2, np.float32)).cuda()
            ws.pairs[k, :N, :] = torch.arange(N, dtype=torch.int32, device="cuda")[:, None]
    ws.npairs[:S] = torch.tensor([len(p1) for p1, _ in sets], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b.estimate_motion()
    return [b.download_motion(k) for k in range(S)]


def run_all(ws, sets):
    out = []
    for k in range(0, len(sets), ws.n_sets):
        out += run_sets(ws, sets[k:k + ws.n_sets])
    return out


def compare(g, o):
    """The assertions of test_estimate_motion for one set, and byte equality of H, F and HorF on top of them: (list of what
    differs, relative deviation of H, of F, bit-identical)."""
    bad = []
    for k in ("flag", "n_h", "n_f"):
        if g[k] != o[k]:
            bad.append("%s %d vs %d" % (k, g[k], o[k]))
    for k in ("mask_h", "mask_f"):
        if not np.array_equal(g[k], o[k]):
            bad.append("%s differs at %s" % (k, np.nonzero(g[k] != o[k])[0][:5].tolist() if len(g[k]) == len(o[k]) else "its length"))
    dev = {}
    for k, tol in (("H", 1e-9), ("F", 1e-9), ("HorF", 1e-6)):
        s = np.abs(o[k]).max()
        d = np.abs(g[k] - o[k]).max()
        dev[k] = d / s if s > 0 else (0.0 if d == 0 else np.inf)
        if not d <= tol * s:                                     # NaN fails; s == 0 (no model) asks for d == 0
            bad.append("%s off by %.3g of max|oracle| = %.3g" % (k, dev[k], s))
    if o["n_h"] == 0 and o["n_f"] == 0:                          # no fit at all: everything stays zero
        if o["flag"] != 0 or any(np.any(g[k] != 0) for k in ("H", "F", "HorF", "mask_h", "mask_f")):
            bad.append("no fit, but an output is not zero")
    same = all(g[k].tobytes() == o[k].tobytes() for k in ("H", "F", "HorF"))
    if not same and not bad:                                     # measured on an MI355X: every set gives the oracle's bytes
        bad.append("within the tolerances, but %s not the oracle's bytes (H off by %.3g, F by %.3g)"
                   % (", ".join(k for k in ("H", "F", "HorF") if g[k].tobytes() != o[k].tobytes()), dev["H"], dev["F"]))
    return bad, dev["H"], dev["F"], same
