"""Shared by test_oracle_stereo.py, test_gpu_stereo.py and tools/fuzz_stereo.py: seeded stereo cases with CRAFTED key points for
Frame::ComputeStereoMatches (k_row_sort / k_stereo_match / k_stereo_filter).  Plain numpy.  A case is one geometry's
(left image, right image, kL, dL, kR, dR): the images only supply the pyramids the SAD windows read, the key points and
descriptors are written, not extracted.  A case's seed depends on its kind, its parameters and its geometry only, never on its
place in a list, so the CPU tests that say which branch a case reaches and the GPU tests that run it speak of the same arrays."""
import itertools

import numpy as np

import __graft_entry__ as graft

KP_DTYPE = graft.load_package().frontend.KP_DTYPE
SEED = 21
F32 = np.float32
TH_HIGH, TH_ORB = 100, 75                 # ORBmatcher::TH_HIGH, (TH_HIGH + TH_LOW) / 2
MARGIN = 8                                # columns of texture left of the left eye's column 0 (negative scene disparities)
SR_ROWS, SR_LEFT, SR_CAND = 16, 128, 256  # k_stereo_match: rows per workgroup, left / right key points per staging pass


def roundf(v):
    """C roundf for v >= 0 (half away from zero); v is f32, so v + 0.5 is exact in f64."""
    return np.floor(np.asarray(v, np.float64) + 0.5)


class Geom:
    """One (W, H, n_levels, scale_factor) with a camera (fx, bf) and the tables the matcher derives from them, formed with
    the roundings of ORBextractor's constructor (csrc/sd_plan.h, sd_params_init / sd_plan_build)."""

    def __init__(self, name, W, H, n_levels, scale_factor, fx, bf, n_features=1200):
        self.name, self.W, self.H, self.n_levels, self.scale_factor = name, W, H, n_levels, scale_factor
        self.fx, self.bf, self.n_features = fx, bf, n_features
        sf = np.float64(F32(scale_factor))
        s = [F32(1.0)]
        for _ in range(1, n_levels):
            s.append(F32(np.float64(s[-1]) * sf))
        self.scale = np.array(s, F32)
        self.inv = F32(1.0) / self.scale
        self.lw = [int(np.rint(F32(W) * i)) for i in self.inv]           # lrintf, like np.rint, rounds halves to even
        self.lh = [int(np.rint(F32(H) * i)) for i in self.inv]
        mb = F32(bf) / F32(fx)
        self.maxD = F32(bf) / mb                                          # Frame.cc:912-915, as the code forms it
        # kp_capacity: sum over levels of the per-level slices (quota + 3 | 4 * nIni) + 1, each rounded up to 8
        factor = F32(1.0 / sf)
        nd = F32(F32(n_features) * (F32(1) - factor)) / F32(F32(1) - F32(np.float64(factor) ** n_levels))
        quota, tot = [], 0
        for _ in range(n_levels - 1):
            quota.append(int(np.rint(nd))); tot += quota[-1]; nd = F32(nd * factor)
        quota.append(max(n_features - tot, 0))
        self.cap = 0
        for l in range(n_levels):
            n_ini = int(roundf(F32(self.lw[l] - 32) / F32(self.lh[l] - 32)))
            self.cap += (max(quota[l] + 3, 4 * n_ini) + 1 + 7) & ~7
        self.band_r = int(np.ceil(F32(2.0) * self.scale[-1])) + 2        # sd_batch_stereo_match's all-level band bound

    def extractor_args(self):
        return (self.n_features, self.scale_factor, self.n_levels, 20, 7)

    def scaled(self, x, level):
        """roundf(x * mvInvScaleFactors[level]) of Frame.cc:965-967, the product in f32."""
        return roundf(np.asarray(x, F32) * self.inv[level])

    def x_for(self, k, level):
        """An f32 x with scaled(x, level) == k."""
        x = F32(F32(k) * self.scale[level])
        for cand in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf)), F32(x + F32(0.25)), F32(x - F32(0.25))):
            if cand >= 0 and self.scaled(cand, level) == k:
                return F32(cand)
        raise AssertionError("no x for column %d of level %d" % (k, level))


# 752 x 240: 15 full 16-row chunks.  1241 x 376: the last chunk is partial.  12 levels = SD_MAX_LEVELS.  5 levels at 2.0:
# bandR = ceil(2 * 16) + 2 = 34 and 16 + 2 * 34 + 2 = 86 <= SD_SR_RS = 96, the widest staged row slice that is accepted (a
# top level needs 62 rows for one FAST cell, hence 1008 rows).
GEOMS = {g.name: g for g in (
    Geom("752x240-8x1.2", 752, 240, 8, 1.2, 435.2046959714599, 47.90639384423901),
    Geom("1241x376-8x1.2", 1241, 376, 8, 1.2, 718.856, 386.1448),
    Geom("1024x500-12x1.2", 1024, 500, 12, 1.2, 517.306408, 40.0),
    Geom("1280x1008-5x2.0", 1280, 1008, 5, 2.0, 718.856, 386.1448),
)}
# refused by sd_batch_stereo_match: 2 * 1.31^11 = 39.0, bandR = 41 or 42, 16 + 2 * bandR + 2 >= 100 > 96.  (6 levels at 2.0 cannot
# be built at all: the top level needs 62 * 32 = 1984 rows and columns, which is more than 4096 FAST cells on level 0.)
REFUSED = Geom("1232x1232-12x1.31", 1232, 1232, 12, 1.31, 718.856, 386.1448)


# ---- domain
# Every byte k_stereo_match loads for a SAD window lies inside the padded plane of its level, for every key point that
# check_domain accepts.  Derivation from csrc/sd_plan.h (border SD_EDGE = 19 rows above and below, interior column 0 at byte
# SD_XOFF = 32 of a row, row stride >= 32 + Wl + 19 + 4 = Wl + 55, Wl = lrintf(W * inv), Hl = lrintf(H * inv)):
#   * 0 <= x < W gives 0 <= x * inv <= W * inv in f32 (the product is monotone), so cL = roundf(x * inv) is in 0 .. Wl + 1
#     (roundf rounds a half up where lrintf rounds it to even, hence the + 1); likewise 0 <= rL = roundf(y * inv) <= Hl + 1.
#   * left window: 12 bytes from column cL - 5, rows rL - 5 .. rL + 5: columns -5 .. Wl + 7 are bytes 27 .. Wl + 39 of a row
#     of at least Wl + 55 bytes; rows -5 .. Hl + 6 lie inside -19 .. Hl + 18.
#   * right window: loaded only when 0 <= cR and cR + 11 < Wl (the iniu / endu guards, evaluated before any address is
#     formed), 24 bytes from column cR - 10: columns -10 .. Wl - 12 - 10 + 23 = Wl + 1, bytes 22 .. Wl + 33; same rows.
#   * x >= 0 makes iniu < 0 unreachable: the right guard that can fire inside the domain is endu >= Wl.
#   * the row tables: (int)y is 0 .. H - 1, octave < n_levels indexes the level tables, count <= kp_capacity <= 65535.
# No corner of the domain had to be narrowed.  Values outside it (negative or non-finite coordinates, octaves beyond the
# level set) are never uploaded: check_domain runs on the host before every launch.
def check_domain(case, cap=None):
    g = case["geom"]
    cap = g.cap if cap is None else cap
    assert case["left"].shape == (g.H, g.W) == case["right"].shape and case["left"].dtype == np.uint8 == case["right"].dtype
    for k, d in ((case["kL"], case["dL"]), (case["kR"], case["dR"])):
        assert k.dtype == KP_DTYPE and d.dtype == np.uint8 and d.shape == (len(k), 32), case["name"]
        assert len(k) <= cap <= 65535, "%s: %d key points, capacity %d" % (case["name"], len(k), cap)
        assert np.isfinite(k["x"]).all() and np.isfinite(k["y"]).all(), case["name"]
        assert ((k["x"] >= 0) & (k["x"] < g.W)).all(), "%s: x outside [0, W)" % case["name"]
        assert ((k["y"] >= 0) & (k["y"] < g.H)).all(), "%s: y outside [0, H)" % case["name"]
        assert ((k["octave"] >= 0) & (k["octave"] < g.n_levels)).all(), "%s: octave outside the level set" % case["name"]
    return case


# ---- images
def _rng(g, *key):
    return np.random.default_rng([SEED, list(GEOMS).index(g.name) if g.name in GEOMS else 99] + [int(k) for k in key])


def _texture(rng, H, Wt):
    """Smooth random texture with structure at 3, 11 and 37 px (every pyramid level sees some), grey levels 23 .. 233."""
    acc = np.zeros((H, Wt))
    for blk, amp in ((3, 40.0), (11, 35.0), (37, 30.0)):
        lo = rng.uniform(-1, 1, (H // blk + 2, Wt // blk + 2))
        acc += amp * np.kron(lo, np.ones((blk, blk)))[:H, :Wt]
    p = np.pad(acc, 1, mode="edge")
    acc = sum(p[i:i + H, j:j + Wt] for i in range(3) for j in range(3)) / 9.0
    return np.clip(np.rint(128 + acc), 0, 255)


_IMAGES = {}
IMAGE_KINDS = ("shift", "copy", "zero", "loud", "flat", "binary")


def images(g, kind, d=0):
    """(left, right) u8.  right[y, x] = left[y, x + d]: a scene at disparity d.  shift: + noise of +-3 grey levels in the right
    eye; copy: none (every SAD at the true shift is 0); loud: noise +-3, and +-30 in the right third of the image; zero: d = 9
    with noise, except a strip mirror-symmetric about column d (sic: d names the column here) that both eyes see unshifted;
    flat: 128 everywhere; binary: 0 / 255 pixels, 2 % of them inverted in the right eye."""
    key = (g.name, kind, d)
    if key in _IMAGES:
        return _IMAGES[key]
    rng = _rng(g, 1, IMAGE_KINDS.index(kind), d + 4096)
    W, H = g.W, g.H
    shift = 9 if kind == "zero" else d
    Wt = MARGIN + W + max(shift, 0) + 1
    tex = _texture(rng, H, Wt)
    if kind == "flat":
        tex[:] = 128
    if kind == "binary":
        tex = 255.0 * (rng.random((H, Wt)) < 0.5)
    left = tex[:, MARGIN:MARGIN + W].copy()
    right = tex[:, MARGIN + shift:MARGIN + shift + W].copy()
    if kind in ("shift", "zero", "loud"):
        right += rng.integers(-3, 4, (H, W))
    if kind == "loud":
        right[:, 2 * W // 3:] += rng.integers(-30, 31, (H, W - 2 * W // 3))
    if kind == "binary":
        flip = rng.random((H, W)) < 0.02
        right[flip] = 255 - right[flip]
    if kind == "zero":
        c, hw = d, 24
        strip = left[:, c - hw:c + hw + 1]
        strip[:, hw + 1:] = strip[:, hw - 1::-1]                          # column c + k == column c - k
        right[:, c - hw:c + hw + 1] = strip
    out = tuple(np.ascontiguousarray(np.clip(im, 0, 255).astype(np.uint8)) for im in (left, right))
    _IMAGES[key] = out
    return out


# ---- key points and descriptors
def kps(g, x, y, octave):
    x = np.atleast_1d(np.asarray(x, F32)); n = len(x)
    k = np.zeros(n, KP_DTYPE)
    k["x"] = x; k["y"] = np.broadcast_to(np.asarray(y, F32), n); k["octave"] = np.broadcast_to(np.asarray(octave, np.int32), n)
    k["size"] = F32(31.0) * g.scale[k["octave"]]; k["response"] = 50.0; k["class_id"] = -1
    return k


def flipped(rng, desc, nbits):
    """desc (N, 32) u8 with exactly nbits[i] bits of row i inverted."""
    desc = np.atleast_2d(desc)
    bits = np.unpackbits(desc, axis=1)
    nb = np.broadcast_to(np.asarray(nbits), len(desc))
    for i in range(len(desc)):
        bits[i, rng.permutation(256)[:nb[i]]] ^= 1
    return np.packbits(bits, axis=1)


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def case(g, name, imgs, kL, dL, kR, dR):
    kL = np.ascontiguousarray(kL, KP_DTYPE); kR = np.ascontiguousarray(kR, KP_DTYPE)
    dL = np.ascontiguousarray(dL, np.uint8).reshape(-1, 32); dR = np.ascontiguousarray(dR, np.uint8).reshape(-1, 32)
    return check_domain(dict(name="%s/%s" % (g.name, name), kind=name.split("-")[0], geom=g, left=imgs[0], right=imgs[1],
                             kL=kL, dL=dL, kR=kR, dR=dR))


def _cat(parts):
    """[(kL, dL, kR, dR)] -> one (kL, dL, kR, dR)."""
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def pairs(g, rng, n, d, level=None, flips=(0, 40), jitter=True, x_lo=None, x_hi=None, y_lo=0, y_hi=None, windowed=True):
    """n left key points with their partners d columns to the left, placed so that the partner's SAD window is accepted
    (0 <= roundf(xR * inv) <= Wl - 12; windowed=False: anywhere in the image).  flips = (lo, hi): bits inverted in the right
    descriptor, uniform in lo .. hi."""
    lv = rng.integers(0, g.n_levels, n) if level is None else np.broadcast_to(np.asarray(level), n).copy()
    s = g.scale[lv].astype(np.float64)
    lwl = np.asarray(g.lw)[lv]
    lo = np.maximum(0.6 * s + 0.5 if windowed else 0.0, (0 if x_lo is None else x_lo) - d)     # bounds of the right x
    hi = np.minimum((lwl - 12.6) * s - 0.5 if windowed else g.W - 1.0, (g.W - 1.0 if x_hi is None else x_hi) - d - 0.5)
    assert (hi > lo).all(), "no room for disparity %d" % d
    xr = rng.uniform(lo, hi, n)
    yl = rng.uniform(y_lo, (g.H if y_hi is None else y_hi) - 1e-3, n)
    if jitter:
        xl = xr + d + rng.uniform(0.0, 0.45, n)
        yr = np.clip(yl + rng.uniform(-1.5, 1.5, n), 0, g.H - 1e-3)
    else:
        xr = np.floor(xr); xl = xr + d; yl = np.floor(yl) + 0.5; yr = yl
    dl = rand_desc(rng, n)
    return kps(g, xl, yl, lv), dl, kps(g, xr, yr, lv), flipped(rng, dl, rng.integers(flips[0], flips[1] + 1, n))


# ---- case kinds
def shifted(g, d, n=300):
    rng = _rng(g, 2, d)
    return case(g, "shifted-d%d" % d, images(g, "shift", d), *pairs(g, rng, n, d, flips=(0, 110)))


def exact_copy(g, d, n=180):
    rng = _rng(g, 3, d)
    # at d != 0 only level 0 sees an exact copy (a shift by d is no shift by a whole number of a coarser level's pixels)
    return case(g, "exact_copy-d%d" % d, images(g, "copy", d), *pairs(g, rng, n, d, level=None if d == 0 else 0))


def zero_disparity_column(g):
    return g.W // 2 + 3


def zero_disparity(g, offset=0.0):
    """40 level-0 key points on the axis of the mirror-symmetric strip in both eyes (the first 40 of the case), 200 ordinary pairs
    elsewhere.  offset moves them off the axis (the CPU test breaks the generator that way to see itself fail)."""
    rng = _rng(g, 4)
    c = zero_disparity_column(g)
    y = rng.permutation(np.arange(8, g.H - 8))[:40] + 0.25
    dl = rand_desc(rng, 40)
    on = (kps(g, np.full(40, c + offset), y, 0), dl, kps(g, np.full(40, c + offset), y, 0), flipped(rng, dl, 5))
    left_part = pairs(g, rng, 100, 9, x_hi=c - 60)
    right_part = pairs(g, rng, 100, 9, x_lo=c + 60)
    return case(g, "zero_disparity", images(g, "zero", c), *_cat([on, left_part, right_part]))


def hamming_thresholds(g):
    """One candidate at a Hamming distance of exactly 74, 75, 99, 100: 12 key points each."""
    rng = _rng(g, 5)
    parts = [pairs(g, rng, 12, 9, flips=(h, h), jitter=False) for h in (74, 75, 99, 100)]
    return case(g, "hamming_thresholds", images(g, "shift", 9), *_cat(parts))


def hamming_ties(g):
    """Groups of 2 .. 5 admissible candidates at the same distance (30 bits) from one left key point, 14 columns apart, the true
    partner among them, in EVERY order of their right indices: the lowest index must win, wherever it lies."""
    rng = _rng(g, 6)
    kL, dL, kR, dR = [], [], [], []
    for n in (2, 3, 4, 5):
        for perm in itertools.permutations(range(n)):
            x = np.floor(rng.uniform(14 * n + 20, g.W - 20)); y = np.floor(rng.uniform(0, g.H)) + 0.5
            d = rand_desc(rng, 1)
            kL.append(kps(g, x, y, 0)); dL.append(d)
            xs = x - 9 - 14.0 * np.asarray(perm)                      # perm[j] == 0: right index j is the true partner
            kR.append(kps(g, xs, y, 0)); dR.append(flipped(rng, np.repeat(d, n, 0), 30))
    return case(g, "hamming_ties", images(g, "shift", 9), *[np.concatenate(a) for a in (kL, dL, kR, dR)])


def hamming_passes(g, low_first):
    """Two candidates at the same distance on the lowest and the highest row of a level-0 key point's band, with 300 unrelated
    right key points on the rows between them: whatever the order inside a row, the row-sorted staging order puts the two
    into different passes of 256 candidates.  low_first: the lower right index is on the lowest row (else on the highest).
    Eight such left key points share the fillers; the true partner is always the lower index."""
    rng = _rng(g, 7, low_first)
    yi = 16 * (g.H // 32) + 7
    x = np.floor(rng.permutation(np.arange(60, g.W - 20, 12))[:8].astype(np.float64))
    dl = rand_desc(rng, 8)
    kL = kps(g, x, yi + 0.5, 0)
    rows = (yi - 2 + 0.5, yi + 2 + 0.5) if low_first else (yi + 2 + 0.5, yi - 2 + 0.5)
    k_true = kps(g, x - 9, rows[0], 0); k_other = kps(g, x - 9 - 14, rows[1], 0)
    fill = kps(g, rng.uniform(0, g.W - 1, 300), rng.uniform(yi - 1, yi + 1.999, 300), rng.integers(0, g.n_levels, 300))
    kR = np.concatenate([k_true, k_other, fill])
    dR = np.concatenate([flipped(rng, dl, 30), flipped(rng, dl, 30), rand_desc(rng, 300)])
    return case(g, "hamming_passes-%s" % ("low" if low_first else "high"), images(g, "shift", 9), kL, dl, kR, dR)


def left_passes(g, n=300):
    """More than two passes of 128 left key points in one 16-row chunk."""
    rng = _rng(g, 8)
    return case(g, "left_passes", images(g, "shift", 9), *pairs(g, rng, n, 9, y_lo=32, y_hi=48))


def octave_gate(g):
    """Left level 0, middle, top; per left key point a candidate on a forbidden level (levelL +- 2) at 10 bits and, 14 columns away,
    one on each admissible level (levelL - 1 .. levelL + 1) at 40 bits; 8 key points per combination."""
    rng = _rng(g, 9)
    parts = []
    for lv in (0, g.n_levels // 2, g.n_levels - 1):
        for bad in (lv - 2, lv + 2):
            for good in (lv - 1, lv, lv + 1):
                if not (0 <= bad < g.n_levels and 0 <= good < g.n_levels):
                    continue
                kL, dL, kR, dR = pairs(g, rng, 8, 9, level=lv, flips=(40, 40), jitter=False)
                kR["octave"] = good
                kB = kR.copy(); kB["octave"] = bad
                kB["x"] = np.where(kR["x"] >= 14 + 2 * g.scale[lv], kR["x"] - 14, kR["x"] + 5)
                parts.append((kL, dL, np.concatenate([kR, kB]), np.concatenate([dR, flipped(rng, dL, 10)])))
    return case(g, "octave_gate", images(g, "shift", 9), *_cat(parts))


def _in_band(y, r, yi):
    """The reference's row-band test (Frame.cc:884-900) in f32: floor(y - r) <= yi <= ceil(y + r)."""
    y = F32(y); r = F32(r)
    return np.floor(F32(y - r)) <= yi <= np.ceil(F32(y + r))


def row_band_edges(g, octave, yi):
    """[(y, inside)] right-eye y values around the two limits of row yi's band for a key point of this octave: the last f32
    inside and the first outside on either side, and y with fractions .999 and .0 next to them."""
    r = F32(2.0) * g.scale[octave]
    out = []
    for start, inward in ((F32(F32(yi + 1) + r), -1), (F32(F32(yi - 1) - r), 1)):
        a, b = F32(start - F32(0.001) * inward), F32(start + F32(0.001) * inward)      # a outside, b inside
        if min(a, b) <= 0:
            continue                                                 # this limit lies above the image
        assert _in_band(b, r, yi) and not _in_band(a, r, yi), "no band limit found"
        ia, ib = int(a.view(np.uint32)), int(b.view(np.uint32))      # positive f32: the bit patterns are ordered like the values
        while abs(ia - ib) > 1:                                      # bisection to the two neighbouring f32 across the limit
            im = (ia + ib) // 2
            if _in_band(np.uint32(im).view(F32), r, yi):
                ib = im
            else:
                ia = im
        prev, y = np.uint32(ia).view(F32), np.uint32(ib).view(F32)
        out += [prev, y]
        base = np.floor(y)
        out += [F32(base + F32(0.999)), F32(base), F32(base - 1 + F32(0.999)), F32(base + 1)]
    return [(F32(y), bool(_in_band(y, r, yi))) for y in out if 0 <= y < g.H]


def row_band(g):
    """For every octave and for left rows 0, 15, 16, H - 1 and the first row of the last chunk: one right key point per band-limit
    value of row_band_edges, each with a left key point of its own at level `octave - 1`: the candidate's radius is then the
    largest that the kernel's per-key-point pre-filter has to allow for (the top octave also gets a left key point of its own
    level, where min(levelL + 1, n_levels - 1) takes the other arm)."""
    rng = _rng(g, 10)
    last = (g.H - 1) // SR_ROWS * SR_ROWS
    parts = []
    for octave in range(g.n_levels):
        for yi in (0, 15, 16, last, g.H - 1):
            for y, _ in row_band_edges(g, octave, yi):
                for lv in {max(octave - 1, 0), octave if octave == g.n_levels - 1 else max(octave - 1, 0)}:
                    kL, dL, kR, dR = pairs(g, rng, 1, 9, level=lv, flips=(20, 20), jitter=False)
                    kL["y"] = yi + 0.5; kR["y"] = y; kR["octave"] = octave
                    parts.append((kL, dL, kR, dR))
    return case(g, "row_band", images(g, "shift", 9), *_cat(parts))


def u_range(g, side):
    """Right x exactly on a limit of [minU, maxU] = [uL - maxD, uL] and one ulp beyond it (10 level-0 key points each).  The scene's
    disparity lies one column inside the limit, so an admitted candidate becomes a match and the GPU output shows the decision.
    side "hi": x = uL and the next f32 above; also 10 key points with uL < maxD (minU < 0) and their candidate at x = 0 .. 1.
    side "lo": x = minU and the next f32 below."""
    rng = _rng(g, 11, side == "lo")
    maxD = g.maxD
    parts = []
    if side == "hi":
        d = 1
        for beyond in (False, True):
            kL, dL, kR, dR = pairs(g, rng, 10, d, level=0, flips=(20, 20), jitter=False)
            kR["x"] = np.nextafter(kL["x"], F32(np.inf)) if beyond else kL["x"]
            parts.append((kL, dL, kR, dR))
        kL, dL, kR, dR = pairs(g, rng, 10, d, level=0, flips=(20, 20), jitter=False, x_hi=float(maxD) - 2)
        parts.append((kL, dL, kR, dR))
    else:
        d = int(np.floor(maxD)) - 1
        for beyond in (False, True):
            kL, dL, kR, dR = pairs(g, rng, 10, d, level=0, flips=(20, 20), jitter=False, x_lo=float(maxD) + 2)
            minU = kL["x"] - maxD
            assert (minU >= 0).all()
            kR["x"] = np.nextafter(minU, F32(-np.inf)) if beyond else minU
            parts.append((kL, dL, kR, dR))
    return case(g, "u_range-%s" % side, images(g, "shift", d), *_cat(parts))


def refine_out_of_range(g, side):
    """Candidates exactly on maxU ("hi", scene disparity -3) or minU ("lo", scene disparity ceil(maxD) + 3): admitted, and the SAD
    refinement then moves bestuR past uL (disparity < 0) or past uL - maxD (disparity >= maxD)."""
    rng = _rng(g, 12, side == "lo")
    if side == "hi":
        d = -3
        kL, dL, kR, dR = pairs(g, rng, 16, d, level=0, flips=(20, 20), jitter=False)
        kR["x"] = kL["x"]
    else:
        d = int(np.ceil(g.maxD)) + 3
        kL, dL, kR, dR = pairs(g, rng, 16, d, level=0, flips=(20, 20), jitter=False, x_lo=float(g.maxD) + 8)
        kR["x"] = kL["x"] - g.maxD
    return case(g, "refine_out_of_range-%s" % side, images(g, "shift", d), kL, dL, kR, dR)


def window_edges(g):
    """Per level, right key points whose scaled column is 0, Wl - 12 (the last accepted: endu = column + 11 < Wl) and Wl - 11 (the
    first refused), 8 each; then level-0 partners moved by -5, +5, -4, +4 columns (the best shift on and beside the edge)."""
    rng = _rng(g, 13)
    parts = []
    for lv in range(g.n_levels):
        for col in (0, g.lw[lv] - 12, g.lw[lv] - 11):
            xr = g.x_for(col, lv)
            y = np.floor(rng.uniform(0, g.H, 8)) + 0.5
            dl = rand_desc(rng, 8)
            parts.append((kps(g, np.full(8, min(float(xr) + 9, g.W - 1)), y, lv), dl, kps(g, np.full(8, xr), y, lv), flipped(rng, dl, 20)))
    for delta in (-5, 5, -4, 4):
        kL, dL, kR, dR = pairs(g, rng, 10, 9, level=0, flips=(20, 20), jitter=False, x_lo=30, x_hi=g.W - 30)
        kR["x"] += delta
        parts.append((kL, dL, kR, dR))
    return case(g, "window_edges", images(g, "shift", 9), *_cat(parts))


def flat_image(g, n=60):
    """All 11 SADs equal (0): the first shift, -5, wins and is an edge shift."""
    rng = _rng(g, 14)
    return case(g, "window_edges-flat", images(g, "flat", 0), *pairs(g, rng, n, 9))


def binary_image(g, n=120):
    """0 / 255 pixels: the largest values the packed u16 SAD lanes see (|(IL - cL) - (IR - cR)| up to 510 per pixel)."""
    rng = _rng(g, 15)
    return case(g, "window_edges-binary", images(g, "binary", 9), *pairs(g, rng, n, 9))


def filter_count(g, n):
    """n exact level-0 pairs (n matches before the median filter) and 6 pairs whose descriptors are 80 bits apart."""
    rng = _rng(g, 16, n)
    good = pairs(g, rng, n, 9, level=0, flips=(10, 10), jitter=False, x_lo=30, x_hi=g.W - 30)
    bad = pairs(g, rng, 6, 9, level=0, flips=(80, 80), jitter=False)
    return case(g, "filter_counts-n%d" % n, images(g, "shift", 9), *_cat([good, bad]))


def filter_duplicates(g):
    """5 distinct pairs and one more whose left key point is there 16 times: the median of the 21 SADs lies inside the run."""
    rng = _rng(g, 17)
    a = pairs(g, rng, 5, 9, level=0, flips=(10, 10), jitter=False, x_lo=30, x_hi=g.W - 30)
    kL, dL, kR, dR = pairs(g, rng, 1, 9, level=0, flips=(10, 10), jitter=False, x_lo=30, x_hi=g.W - 30)
    return case(g, "filter_counts-duplicates", images(g, "shift", 9), *_cat([a, (np.repeat(kL, 16), np.repeat(dL, 16, 0), kR, dR)]))


def filter_both_sides(g, n=240):
    """Pairs over an image whose right third is much noisier: SADs on both sides of 2.1 x median."""
    rng = _rng(g, 18)
    return case(g, "filter_counts-loud", images(g, "loud", 9), *pairs(g, rng, n, 9, flips=(0, 30)))


def counts(g, n_left, n_right, cap=None):
    """min(n_left, n_right) pairs, the larger side filled up with unrelated key points."""
    cap = g.cap if cap is None else cap
    rng = _rng(g, 19, n_left, n_right)
    n = min(n_left, n_right)
    kL, dL, kR, dR = pairs(g, rng, n, 9)
    extra = max(n_left, n_right) - n
    ke = kps(g, rng.uniform(0, g.W - 1, extra), rng.uniform(0, g.H - 1e-3, extra), rng.integers(0, g.n_levels, extra)); de = rand_desc(rng, extra)
    if n_left > n:
        kL, dL = np.concatenate([kL, ke]), np.concatenate([dL, de])
    else:
        kR, dR = np.concatenate([kR, ke]), np.concatenate([dR, de])
    c = case(g, "counts-%dx%d" % (n_left, n_right), images(g, "shift", 9), kL, dL, kR, dR)
    return check_domain(c, cap)


SHIFTS = (0, 1, 9, 40, 200)
FILTER_COUNTS = (0, 1, 2, 3, 40, 41)


def suite(g):
    """Every case kind at geometry g."""
    cap = g.cap
    out = [shifted(g, d) for d in SHIFTS]
    out += [exact_copy(g, 0), exact_copy(g, 9), zero_disparity(g)]
    out += [hamming_thresholds(g), hamming_ties(g), hamming_passes(g, True), hamming_passes(g, False), left_passes(g)]
    out += [octave_gate(g), row_band(g), u_range(g, "hi"), u_range(g, "lo")]
    out += [window_edges(g), flat_image(g), binary_image(g), refine_out_of_range(g, "hi"), refine_out_of_range(g, "lo")]
    out += [filter_count(g, n) for n in FILTER_COUNTS] + [filter_duplicates(g), filter_both_sides(g)]
    out += [counts(g, a, b) for a, b in ((0, 50), (50, 0), (0, 0), (1, 1), (cap - 1, cap - 1), (cap, cap), (cap, 1), (1, cap))]
    return out


# ---- the oracle side
_EXTRACTORS = {}


def oracle_extractors(orc, c):
    """The oracle extractors that hold the pyramids of the case's two images (cached per image)."""
    out = []
    for im in (c["left"], c["right"]):
        key = (c["geom"].name, id(im))
        if key not in _EXTRACTORS:
            e = orc.Extractor(*c["geom"].extractor_args())
            e(im)
            _EXTRACTORS[key] = (e, im)                               # the image is kept alive: its id stays its own
        out.append(_EXTRACTORS[key][0])
    return out


def oracle(orc, c):
    g = c["geom"]
    eL, eR = oracle_extractors(orc, c)
    return orc.stereo_matches_ex(eL, eR, c["kL"], c["dL"], c["kR"], c["dR"], g.bf, g.fx)


def histogram(results):
    h = np.zeros(10, np.int64)
    for r in results:
        h += np.bincount(r["outcome"], minlength=10)
    return h


# ---- the device side (tests marked gpu and tools/fuzz_stereo.py): crafted arrays written over a workspace's extraction results

class Workspace:
    """2 * n_frames image slots of one geometry: slots 2f / 2f + 1 are the left / right eye of frame f."""

    def __init__(self, fe, g, n_frames):
        self.fe, self.g, self.n_frames = fe, g, n_frames
        self.ex = fe.ORBextractor(*g.extractor_args())
        self.b = fe.Batch(self.ex, g.W, g.H, 2 * n_frames)
        kp_p, desc_p, cnt_p, self.cap = self.b.results_device()
        n = 2 * n_frames
        self.kp = fe.as_torch_u8(kp_p, n * self.cap * KP_DTYPE.itemsize).view(n, self.cap * KP_DTYPE.itemsize)
        self.desc = fe.as_torch_u8(desc_p, n * self.cap * 32).view(n, self.cap * 32)
        import torch
        self.count = fe.as_torch_u8(cnt_p, n * 4).view(torch.int32)

    def close(self):
        self.b.close()


def run_cases(ws, cases, check_pyramids=None):
    """The device matcher on len(cases) cases in ONE launch: one extract_host of the cases' image pairs builds the pyramids (and
    marks the slots extracted), then case f's key points, descriptors and counts overwrite slots 2f, 2f + 1; stereo_match;
    download.  -> [(mvuRight, mvDepth, sad)] cut to the case's left count.  check_pyramids(f, case, batch), if given, runs
    before the match."""
    import torch
    b, F = ws.b, len(cases)
    assert 0 < F <= ws.n_frames
    for c in cases:
        assert c["geom"] is ws.g
        check_domain(c, ws.cap)
    b.extract_host(np.stack([im for c in cases for im in (c["left"], c["right"])]))
    b.sync()
    counts_ = []
    for f, c in enumerate(cases):
        for slot, k, d in ((2 * f, c["kL"], c["dL"]), (2 * f + 1, c["kR"], c["dR"])):
            if len(k):
                ws.kp[slot, :k.nbytes] = torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda()
                ws.desc[slot, :d.size] = torch.from_numpy(d.reshape(-1).copy()).cuda()
            counts_.append(len(k))
    ws.count[:2 * F] = torch.tensor(counts_, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if check_pyramids is not None:
        for f, c in enumerate(cases):
            check_pyramids(f, c, b)
    b.stereo_match(F, ws.g.bf, ws.g.fx)
    out = []
    for f, c in enumerate(cases):
        ur, dep, sad = b.download_stereo(f)
        n = len(c["kL"])
        out.append((ur[:n].copy(), dep[:n].copy(), sad[:n].copy()))
    return out


def compare(got, o):
    """Byte equality of mvuRight, mvDepth and the SAD array with the oracle's: the list of what differs."""
    ur, dep, sad = got
    bad = []
    for name, a, b in (("sad", sad, o["sad"]), ("mvuRight", ur.view(np.uint32), o["ur"].view(np.uint32)),
                       ("mvDepth", dep.view(np.uint32), o["dep"].view(np.uint32))):
        if not np.array_equal(a, b):
            i = np.nonzero(a != b)[0]
            bad.append("%s differs at %d of %d left key points, first %d (oracle outcome %d): %r vs %r"
                       % (name, len(i), len(a), i[0], o["outcome"][i[0]], a[i[0]], b[i[0]]))
    return bad
