"""Shared by test_extract_cases.py, test_gpu_extract_cases.py and test_oracle_leaves.py: CRAFTED images for
the ORB extractor (k_pyr_level*, k_fast_cells_staged / k_fast_cells, k_quadtree, k_orient, k_blur*, k_describe) and a plain numpy
restatement of each stage from its definition.  Every builder returns a list of Shot(name, img, params, cases); a case is
(name, level, (x, y), claim): the claim is what the oracle must show at that pixel of that level (test_extract_cases.witness),
optionally with the name of the "wrong twin" rule that must give another result on the same image.

The restatement takes one switch per rule that turns the rule into its neighbour (TWINS).  It pins the oracle on the crafted
images; the device is compared with the oracle, byte for byte."""
import math
import os
import re
from collections import namedtuple

import numpy as np

F32 = np.float32
Shot = namedtuple("Shot", "name img params cases")      # params = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
Case = namedtuple("Case", "name level xy claim")

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3)]                      # (dx, dy), cv::FAST's order; compass points are 0, 4, 8, 12
EDGE = 19                                               # EDGE_THRESHOLD
TRUE = dict(score_ge=True, nms_strict=True, retry_after_nms=True, nms_in_cell=True, tie_first=True, desc_lt=True,
            round_even=True)
TWINS = {"score_gt": dict(score_ge=False),              # corner iff score > T          (true: score >= T)
         "nms_ge": dict(nms_strict=False),              # maximum iff s >= neighbours   (true: s > neighbours)
         "retry_before_nms": dict(retry_after_nms=False),   # retry iff no corner BEFORE NMS (true: no key point after NMS)
         "nms_across": dict(nms_in_cell=False),         # NMS sees the scores of the next cell (true: zero outside the scanned area)
         "tie_last": dict(tie_first=False),             # last of equal responses in a node (true: first in candidate order)
         "desc_le": dict(desc_lt=False),                # bit = t0 <= t1                (true: t0 < t1)
         "round_away": dict(round_even=False)}          # taps round half away from zero (true: half to even)


def rules(twin=None):
    r = dict(TRUE)
    if twin:
        r.update(TWINS[twin])
    return r


# ------------------------------------------------------------------------------------------------ the restatement
def fast_score(img):
    """FAST-9/16 from its definition: score(p) = the largest t for which >= 9 contiguous ring pixels are all darker than v - t or
    all brighter than v + t (0 where there is none, and in the 3-px frame the ring does not fit in)."""
    I = np.asarray(img).astype(np.int32)
    h, w = I.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    v = I[3:h - 3, 3:w - 3]
    d = np.stack([v - I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    best = np.zeros_like(v)
    for sign in (1, -1):
        s = np.concatenate([sign * d, sign * d[:8]])
        for k in range(16):
            best = np.maximum(best, s[k:k + 9].min(0))      # every ring pixel of this arc differs by more than t  <=>  t < the arc's minimum
    out[3:h - 3, 3:w - 3] = np.maximum(best - 1, 0)
    return out


def nms(sc, strict=True, outside=None):
    """3x3 maximum over a score map.  Outside the map: zero, or the scores of `outside` = (larger map, y0, x0)."""
    h, w = sc.shape
    if outside is None:
        P = np.zeros((h + 2, w + 2), np.int32); P[1:-1, 1:-1] = sc
    else:
        big, y0, x0 = outside
        B = np.zeros((big.shape[0] + 2, big.shape[1] + 2), np.int32); B[1:-1, 1:-1] = big
        P = B[y0:y0 + h + 2, x0:x0 + w + 2].copy()
        P[4:-4, 4:-4] = sc[3:-3, 3:-3]                  # the window's own 3-px frame is where the next cell scans
    keep = sc > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                nb = P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                keep &= (sc > nb) if strict else (sc >= nb)
    return keep


def brute_fast(img, thr, twin=None, outside=None):
    """cv::FAST(img, thr, nonmaxSuppression = true): int32 rows (x, y, score) in row-major order."""
    R = rules(twin)
    sc = fast_score(img)
    sc = np.where(sc >= thr if R["score_ge"] else sc > thr, sc, 0)
    if outside is not None:
        big, y0, x0 = outside
        outside = (np.where(big >= thr if R["score_ge"] else big > thr, big, 0), y0, x0)
    keep = nms(sc, R["nms_strict"], outside)
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys, sc[ys, xs]], 1).astype(np.int32).reshape(-1, 3)


def cell_grid(W, H):
    """ORBextractor::ComputeKeyPointsOctTree's 30-px cell windows of a W x H level: (x0, y0, x1, y1, j * wCell, i * hCell)."""
    minB, maxBX, maxBY = EDGE - 3, W - EDGE + 3, H - EDGE + 3
    width, height = F32(maxBX - minB), F32(maxBY - minB)
    nCols, nRows = int(width / F32(30)), int(height / F32(30))
    cells = []
    if nCols < 1 or nRows < 1:
        return cells
    wCell, hCell = int(math.ceil(width / F32(nCols))), int(math.ceil(height / F32(nRows)))
    for i in range(nRows):
        iniY = minB + i * hCell
        if iniY >= maxBY - 3:
            continue
        maxY = min(iniY + hCell + 6, maxBY)
        for j in range(nCols):
            iniX = minB + j * wCell
            if iniX >= maxBX - 6:
                continue
            cells.append((iniX, iniY, min(iniX + wCell + 6, maxBX), maxY, j * wCell, i * hCell))
    return cells


def detect(plane, ini, mn, twin=None, per_cell=None):
    """The FAST candidates of one level's interior plane: per cell FAST at iniTh, and at minTh where that left no key point.
    int32 rows (x, y, response) in level coordinates, cells in row-major order (the order DistributeOctTree receives)."""
    R = rules(twin)
    H, W = plane.shape
    out = []
    big = None if R["nms_in_cell"] else fast_score(plane)
    for x0, y0, x1, y1, jw, ih in cell_grid(W, H):
        sub = plane[y0:y1, x0:x1]
        if big is not None:
            # the twin's scores next door: those of the whole plane, but only where SOME cell scans (the outermost frame stays zero)
            m = np.zeros_like(big); m[EDGE:H - EDGE, EDGE:W - EDGE] = big[EDGE:H - EDGE, EDGE:W - EDGE]
            outside = (m, y0, x0)
        else:
            outside = None
        r = brute_fast(sub, ini, twin, outside)
        if R["retry_after_nms"]:
            again = len(r) == 0
        else:
            s = fast_score(sub)
            again = not ((s >= ini) if R["score_ge"] else (s > ini)).any()
        if again and mn != ini:
            r = brute_fast(sub, mn, twin, outside)
        if per_cell is not None:
            per_cell.append(len(r))
        for x, y, s in r:
            out.append((x + x0, y + y0, s))
    return np.array(out, np.int32).reshape(-1, 3)


def umax_table():
    """ORBextractor's umax: the half width of the circular 31-px patch per row."""
    u = [0] * 16
    vmax = int(math.floor(15 * math.sqrt(2.0) / 2 + 1)); vmin = int(math.ceil(15 * math.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        u[v] = int(np.rint(math.sqrt(225.0 - v * v)))
    v0 = 0
    for v in range(15, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0; v0 += 1
    return u


UMAX = umax_table()


def moments(padded, x, y):
    """IC_Angle's (m01, m10) at interior pixel (x, y) of a plane padded by 19 px."""
    I = padded.astype(np.int64)
    cy, cx = y + EDGE, x + EDGE
    m01 = m10 = 0
    for v in range(-15, 16):
        d = UMAX[abs(v)]
        row = I[cy + v, cx - d:cx + d + 1]
        m10 += int((np.arange(-d, d + 1) * row).sum()); m01 += v * int(row.sum())
    return m01, m10


def reflect_pad(plane):
    return np.pad(plane, EDGE, mode="reflect")          # BORDER_REFLECT_101


_PATTERN = None


def pattern():
    """bit_pattern_31_ as int array [256][4] = (x0, y0, x1, y1)."""
    global _PATTERN
    if _PATTERN is None:
        here = os.path.dirname(os.path.abspath(__file__))
        with open(os.path.join(here, "..", "oracle", "orb_pattern.inc")) as f:
            txt = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
        v = np.array([int(t) for t in re.findall(r"-?\d+", txt)], np.int32)
        assert v.size == 1024
        _PATTERN = v.reshape(256, 4)
    return _PATTERN


def cos_sin(angle):
    """a, b of computeOrbDescriptor: the f32 cos / sin of the f32 angle in radians."""
    rad = F32(F32(angle) * F32(math.pi / F32(180.0)))
    return F32(math.cos(float(rad))), F32(math.sin(float(rad)))


def round_tap(v, even=True):
    v = np.asarray(v, np.float64)
    return (np.rint(v) if even else np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def tap_coords(angle, twin=None):
    """Rounded (dx, dy) of the 512 pattern points at a key point angle, [256][2][2], and the unrounded f32 values."""
    R = rules(twin)
    a, b = cos_sin(angle)
    P = pattern().reshape(256, 2, 2).astype(np.float32)
    x, y = P[..., 0], P[..., 1]
    fx = (x * a).astype(np.float32) - (y * b).astype(np.float32)          # x * a - y * b, two roundings per product-sum
    fy = (x * b).astype(np.float32) + (y * a).astype(np.float32)
    return np.stack([round_tap(fx, R["round_even"]), round_tap(fy, R["round_even"])], -1), np.stack([fx, fy], -1)


def describe(blurred, x, y, angle, twin=None):
    """computeOrbDescriptor at interior pixel (x, y) of the blurred plane: 32 bytes."""
    R = rules(twin)
    t, _ = tap_coords(angle, twin)
    val = blurred[y + t[..., 1], x + t[..., 0]].astype(np.int32)           # [256][2]
    bits = (val[:, 0] < val[:, 1]) if R["desc_lt"] else (val[:, 0] <= val[:, 1])
    return np.packbits(bits.astype(np.uint8), bitorder="little")


def pick(cands, twin=None):
    """The key point a quadtree node keeps: the largest response, the first (twin: the last) of equals in candidate order."""
    r = cands[:, 2]
    i = int(np.argmax(r)) if rules(twin)["tie_first"] else len(r) - 1 - int(np.argmax(r[::-1]))
    return cands[i]


def quadtree(c, W, H, N, twin=None):
    """ORBextractor::DistributeOctTree over the candidates c = rows (x, y, response) of a W x H level, in candidate order: the rows it
    keeps, in its output order.  Node order as the std::list has it (children pushed to the front), the sorted pass by (size, creation
    sequence), the result per node by pick()."""
    minB, w, h = EDGE - 3, W - 2 * (EDGE - 3), H - 2 * (EDGE - 3)
    nIni = int(math.floor(float(F32(w) / F32(h)) + 0.5))
    if nIni < 1 or len(c) == 0:
        return c[:0]
    hX = F32(w) / F32(nIni)
    X, Y = c[:, 0] - minB, c[:, 1] - minB
    seq = [0]

    def node(x0, x1, y0, y1, idx):
        seq[0] += 1
        return dict(x0=x0, x1=x1, y0=y0, y1=y1, idx=idx, seq=seq[0])

    def divide(n):
        hx = int(math.ceil(float(F32(n["x1"] - n["x0"]) / F32(2)))); hy = int(math.ceil(float(F32(n["y1"] - n["y0"]) / F32(2))))
        mx, my = n["x0"] + hx, n["y0"] + hy
        i = n["idx"]
        L, T = X[i] < mx, Y[i] < my
        return [node(*r, i[m]) for r, m in (((n["x0"], mx, n["y0"], my), L & T), ((mx, n["x1"], n["y0"], my), ~L & T),
                                            ((n["x0"], mx, my, n["y1"]), L & ~T), ((mx, n["x1"], my, n["y1"]), ~L & ~T)) if m.any()]

    ini = (X.astype(np.float32) / hX).astype(np.int64)
    nodes = [node(int(hX * F32(i)), int(hX * F32(i + 1)), 0, h, np.nonzero(ini == i)[0]) for i in range(nIni)]
    nodes = [n for n in nodes if len(n["idx"])]
    while True:
        prev = len(nodes)
        fresh, kept, expand = [], [], []
        for n in nodes:
            if len(n["idx"]) == 1:
                kept.append(n)
                continue
            ch = divide(n)
            fresh = ch[::-1] + fresh                                            # push_front, one by one
            expand += [k for k in ch if len(k["idx"]) > 1]
        nodes = fresh + kept
        if len(nodes) >= N or len(nodes) == prev:
            break
        if len(nodes) + 3 * len(expand) > N:
            done = False
            while not done:
                prev = len(nodes)
                order = sorted(expand, key=lambda n: (len(n["idx"]), n["seq"]))
                expand = []
                for n in order[::-1]:
                    ch = divide(n)
                    nodes = ch[::-1] + [k for k in nodes if k is not n]
                    expand += [k for k in ch if len(k["idx"]) > 1]
                    if len(nodes) >= N:
                        break
                done = len(nodes) >= N or len(nodes) == prev
            break
    return np.array([pick(c[n["idx"]], twin) for n in nodes], np.int32).reshape(-1, 3)


def level_sizes(W, H, scale, nlevels):
    """(W, H) of every pyramid level with the roundings of ORBextractor's constructor and ComputePyramid (csrc/sd_plan.h)."""
    sf = float(F32(scale))
    s, out = F32(1), []
    for l in range(nlevels):
        if l:
            s = F32(float(s) * sf)
        inv = F32(1) / s
        out.append((int(np.rint(F32(W) * inv)), int(np.rint(F32(H) * inv))))
    return out


PT_TW, PT_TH, PT_XSHIFT, PT_LDS = 256, 16, 5, 48 * 1024    # SD_PT_TW, SD_PT_TH, SD_PT_XSHIFT and the LDS budget of k_pyr_level_tiles


def pyr_paths(W, H, scale, nlevels):
    """Which pyramid kernel each level >= 1 of a W x H image takes, restated from ensure_pyr_tiles (csrc/sd_api.hip): rows
    (level, padded width, padded height, tilesX, tilesY, tiles) with tiles = True for k_pyr_level_tiles, whose 256 x 16 tiles lie
    over the level's padded plane shifted 5 px left, and False for the per-thread k_pyr_level, taken when the source rows and
    columns of the largest tile do not fit into 48 KiB of LDS."""
    lv = level_sizes(W, H, scale, nlevels)

    def refl(p, n):
        p = np.abs(p)
        return np.where(p >= n, 2 * (n - 1) - p, p)

    out = []
    for l in range(1, nlevels):
        (sW, sH), (gW, gH) = lv[l - 1], lv[l]
        PW, HP = gW + 2 * EDGE, gH + 2 * EDGE
        sx = np.floor(((np.arange(gW) + 0.5) * (1.0 / (gW / sW)) - 0.5).astype(np.float32)).astype(np.int64)     # OpenCV's xofs
        sx = np.where(sx < 0, 0, np.where(sx >= sW - 1, sW - 1, sx))
        sy = np.floor(((np.arange(gH) + 0.5) * (1.0 / (gH / sH)) - 0.5).astype(np.float32)).astype(np.int64)     # yofs, unclamped
        tilesX, tilesY = (PW + PT_XSHIFT + PT_TW - 1) // PT_TW, (HP + PT_TH - 1) // PT_TH
        spanX = spanY = 0
        for tx in range(tilesX):
            c = sx[refl(np.clip(tx * PT_TW - PT_XSHIFT + np.arange(PT_TW), 0, PW - 1) - EDGE, gW)]
            spanX = max(spanX, int(c.max() - c.min()) + 2)
        for ty in range(tilesY):
            r = sy[refl(np.minimum(ty * PT_TH + np.arange(PT_TH), HP - 1) - EDGE, gH)]
            spanY = max(spanY, int(np.clip(r + 1, 0, sH - 1).max() - np.clip(r, 0, sH - 1).min()) + 1)
        lds = spanY * ((spanX + 16 + 15) & ~15) + spanY * PT_TW * 2
        out.append((l, PW, HP, tilesX, tilesY, bool(lds <= PT_LDS and gW >= 40 and gH >= 40)))
    return out


# ------------------------------------------------------------------------------------------------ canvases
# Both FAST kernels see every FAST / NMS / retry case: the batch runs k_fast_cells_staged when no FAST window of any level is
# wider than 52 px, else the generic k_fast_cells.  200 x 150, one level: 5 x 3 cells of 34 x 40 (+6) -> staged.
# 120 x 100 with a second level at 1.4 (86 x 71: ONE cell, 54 + 6 = 60 px wide) -> generic, and level 0 still has 2 x 2 cells
# (44 x 34), so cell borders and a cell corner exist there too.
Canvas = namedtuple("Canvas", "name W H scale nlevels")
STAGED = Canvas("staged", 200, 150, 1.2, 1)
GENERIC = Canvas("generic", 120, 100, 1.4, 2)
CANVASES = (STAGED, GENERIC)


def scan_areas(W, H):
    """Per cell the scanned pixels [sx0, sx1) x [sy0, sy1) in level coordinates (FAST skips a 3-px frame of its window)."""
    return [(x0 + 3, y0 + 3, x1 - 3, y1 - 3) for x0, y0, x1, y1, _, _ in cell_grid(W, H)]


def params(cv, nf, ini, mn):
    return (nf, cv.scale, cv.nlevels, ini, mn)


def ring_tile(v, ring, bg):
    """7 x 7 values: centre v, the 16 ring pixels as given, the rest bg."""
    t = np.full((7, 7), bg, np.int32)
    for (dx, dy), r in zip(RING, ring):
        t[3 + dy, 3 + dx] = r
    t[3, 3] = v
    return t


class Sheet:
    """Places small tiles on a flat canvas, one per slot, slots `pitch` px apart inside the scanned area, x mod 4 varied by a
    per-row stagger; a new image when one is full."""

    def __init__(self, cv, bg, pitch=11):
        self.cv, self.bg, self.pitch = cv, bg, pitch
        self.imgs, self.cases = [], []
        self._new()

    def _new(self):
        self.imgs.append(np.full((self.cv.H, self.cv.W), self.bg, np.uint8)); self.cases.append([])
        self.row, self.col = 0, 0

    def slot(self):
        cv, p = self.cv, self.pitch
        while True:
            x = EDGE + 4 + self.col * p + (self.row * 3 + self.col) % 4          # every x mod 4 occurs
            y = EDGE + 4 + self.row * p
            if x > cv.W - EDGE - 6:
                self.row += 1; self.col = 0
                continue
            if y > cv.H - EDGE - 6:
                self._new()
                continue
            self.col += 1
            return x, y

    def put(self, tile, name, claim, at=None):
        """Centre of `tile` (odd size) at the next slot (or at `at`); returns the centre."""
        x, y = at if at is not None else self.slot()
        r = tile.shape[0] // 2
        self.imgs[-1][y - r:y + r + 1, x - r:x + r + 1] = np.clip(tile, 0, 255).astype(np.uint8)
        self.cases[-1].append(Case(name, 0, (x, y), claim))
        return x, y

    def shots(self, name, prm):
        return [Shot("%s/%s/%d" % (name, self.cv.name, i), im, prm, cs) for i, (im, cs) in enumerate(zip(self.imgs, self.cases)) if cs]


def block_tile(v, ring, size=13):
    """A size x size block of v with the centre's ring as given: the centre's 3 x 3 neighbours see only the block and a few ring pixels."""
    t = np.full((size, size), v, np.int32)
    t[size // 2 - 3:size // 2 + 4, size // 2 - 3:size // 2 + 4] = ring_tile(v, ring, v)
    return t


def kp_claim(score, T):
    return ("cand", score) if score >= T else ("no_cand",)


# ------------------------------------------------------------------------------------------------ threshold_edges
def threshold_edges():
    """Isolated pixels whose score is exactly T - 1, T, T + 1 for both polarities and all parities of (v, bg, T), the saturation
    pairs at both ends of the byte range, the `both` branch of phase 2, and 8 / 9 contiguous ring pixels at all 16 rotations."""
    shots = []
    for cv in CANVASES:
        for T in (20, 7):                                                   # both parities of T; iniTh == minTh == T: one pass decides
            for bg0 in (60, 61):                                            # both parities of the background
                sh = Sheet(cv, bg0)
                bl = Sheet(cv, bg0, pitch=17)
                for sgn, pol in ((1, "bright"), (-1, "dark")):
                    for s in (T - 1, T, T + 1, T + 2):                      # v = bg +- (s + 1): both parities of v for each bg, T
                        v = bg0 + sgn * (s + 1)
                        tw = "score_gt" if s == T else None
                        sh.put(ring_tile(v, [bg0] * 16, bg0), "%s score %d at T=%d bg=%d" % (pol, s, T, bg0), kp_claim(s, T) + ((tw,) if tw else ()))
                # 16-ring with exactly 8 and exactly 9 contiguous qualifying pixels at each rotation, both polarities: the arc is
                # T + 1 away from the centre (score T), the other ring pixels equal the centre
                for sgn, pol in ((1, "bright"), (-1, "dark")):
                    for n in (8, 9):
                        for rot in range(16):
                            v = bg0 + sgn * (T + 1)
                            ring = [v] * 16
                            for k in range(n):
                                ring[(rot + k) % 16] = bg0
                            bl.put(block_tile(v, ring), "%s %d-arc rot %d T=%d" % (pol, n, rot, T), ("cand", T, "score_gt") if n == 9 else ("no_cand",))
                # the `both` branch: two compass points darker than v - T and two brighter than v + T; the 9-arc (ring 15 .. 7,
                # compass 0 and 4) in one polarity, compass 8 and 12 in the other
                for sgn, pol in ((1, "dark arc (tried first)"), (-1, "bright arc (tried second)")):
                    v = 128 + (bg0 & 1)
                    ring = [v] * 16
                    for k in range(9):
                        ring[(15 + k) % 16] = v - sgn * (T + 1)
                    ring[8] = ring[12] = v + sgn * (T + 30)
                    bl.put(block_tile(v, ring), "both compass polarities, %s T=%d" % (pol, T), ("cand", T, "score_gt"))
                shots += sh.shots("threshold_edges T=%d bg=%d" % (T, bg0), params(cv, 500, T, T))
                shots += bl.shots("threshold_edges arcs T=%d bg=%d" % (T, bg0), params(cv, 500, T, T))
        # saturation: v - T < 0 and v + T > 255 must not lose or invent a corner (byte-wise borrow guards of the halved test)
        T = 20
        for bg, v, s in ((234, 255, 20), (235, 255, 19), (0, 20, 19), (0, 21, 20), (20, 0, 19), (21, 0, 20), (255, 234, 20), (255, 235, 19),
                         (0, 255, 254), (255, 0, 254), (1, 0, 0), (254, 255, 0), (10, 0, 9), (245, 255, 9)):
            sh = Sheet(cv, bg)
            for k, (qx, qy) in enumerate(((1, 1), (3, 1), (1, 3), (3, 3))):     # one per quadrant of the quadtree's root, every x mod 4
                sh.put(ring_tile(v, [bg] * 16, bg), "saturation v=%d on bg=%d: score %d at T=20" % (v, bg, s),
                       kp_claim(s, T) + (("score_gt",) if s == T else ()), at=(qx * cv.W // 4 + k, qy * cv.H // 4))
            shots += sh.shots("threshold_edges sat bg=%d v=%d" % (bg, v), params(cv, 500, T, T))
    return shots


# ------------------------------------------------------------------------------------------------ nms_ties
NB8 = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def _pair(img, x, y, dx, dy, a, b, bg=60):
    img[y, x] = bg + a + 1; img[y + dy, x + dx] = bg + b + 1


def nms_ties():
    """Adjacent corners (two raised pixels: each is a corner whose score is its own height - 1, the other lies inside the ring)
    with equal scores and scores differing by 1 in all 8 directions; pairs straddling a cell border horizontally, vertically and
    at a cell corner; maxima in the first and last scanned column and row of a cell."""
    shots = []
    for cv in CANVASES:
        img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
        areas = scan_areas(cv.W, cv.H)
        # slots 9 px apart, at least 5 px inside their cell's scanned area (a pair reaches 1 px further)
        all_slots = []
        for (bx0, by0, bx1, by1) in areas:
            all_slots += [(bx0 + 5 + 9 * i, by0 + 5 + 9 * j) for j in range((by1 - by0 - 8) // 9) for i in range((bx1 - bx0 - 8) // 9)]
        it = iter(all_slots)
        for dx, dy in NB8:
            x, y = next(it)
            _pair(img, x, y, dx, dy, 50, 50)
            cases.append(Case("equal scores, neighbour (%d,%d): both cancel" % (dx, dy), 0, (x, y), ("no_cand", "nms_ge")))
            cases.append(Case("equal scores, neighbour (%d,%d): both cancel (the other)" % (dx, dy), 0, (x + dx, y + dy), ("no_cand", "nms_ge")))
            x, y = next(it)
            _pair(img, x, y, dx, dy, 51, 50)
            cases.append(Case("scores 51 / 50, neighbour (%d,%d): the larger stays" % (dx, dy), 0, (x, y), ("cand", 51)))
            cases.append(Case("scores 51 / 50, neighbour (%d,%d): the smaller goes" % (dx, dy), 0, (x + dx, y + dy), ("no_cand",)))
        shots.append(Shot("nms_ties/pairs/%s" % cv.name, img, params(cv, 500, 20, 7), cases))

        # cell borders.  Scanned areas of neighbouring cells are contiguous: the last scanned column of cell j is x1 - 4, the first
        # of cell j + 1 is x1 - 3.  Equal scores on both sides: each is the maximum of ITS cell (zero frame) -> both stay.
        img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
        a = areas[0]
        xb, yb = a[2], a[3]                                                   # first scanned column / row of the next cell
        ym, xm = (a[1] + a[3]) // 2, (a[0] + a[2]) // 2
        for nm, (x, y, dx, dy) in (("horizontal", (xb - 1, ym, 1, 0)), ("vertical", (xm, yb - 1, 0, 1)), ("cell corner", (xb - 1, yb - 1, 1, 1))):
            _pair(img, x, y, dx, dy, 50, 50)
            cases.append(Case("equal pair across the %s cell border: both stay" % nm, 0, (x, y), ("cand", 50, "nms_across")))
            cases.append(Case("equal pair across the %s cell border: both stay (the other)" % nm, 0, (x + dx, y + dy), ("cand", 50, "nms_across")))
        # 51 / 50 across the border further along: the smaller one stays too
        _pair(img, xb - 1, ym - 12, 1, 0, 51, 50)
        cases.append(Case("51 | 50 across the horizontal border: the smaller stays in its own cell", 0, (xb, ym - 12), ("cand", 50, "nms_across")))
        shots.append(Shot("nms_ties/borders/%s" % cv.name, img, params(cv, 500, 20, 7), cases))

        # maxima in the first and last scanned column and row of a cell (the last cell too: the image's own limit)
        img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
        for ci, (bx0, by0, bx1, by1) in ((0, areas[0]), (len(areas) - 1, areas[-1])):
            mx, my = (bx0 + bx1) // 2, (by0 + by1) // 2
            for nm, (x, y) in (("first column", (bx0, my)), ("last column", (bx1 - 1, my + 8)), ("first row", (mx, by0)), ("last row", (mx + 8, by1 - 1)),
                               ("first row and column", (bx0, by0)), ("last row and column", (bx1 - 1, by1 - 1))):
                img[y, x] = 200
                cases.append(Case("maximum in the %s of cell %d" % (nm, ci), 0, (x, y), ("cand", 139)))
        shots.append(Shot("nms_ties/rims/%s" % cv.name, img, params(cv, 500, 20, 7), cases))
    return shots


# ------------------------------------------------------------------------------------------------ retry
RETRY_OFF = ((9, 10), (0, 10))                         # the second and third pixel of a retry cell, from its first


def retry():
    """The iniTh -> minTh rule per cell: a tie-cancel cell, a cell with sub-iniTh corners only, a cell with one iniTh corner plus weaker
    ones, and the same with iniTh == minTh.  A cell that shares an edge with each of them stays empty and is claimed to hold no candidate
    (the retry of one cell must not leak into the next).  The staged canvas (5 x 3 cells) holds all three in one image; the generic one (2 x 2
    cells) has one free edge neighbour only for two of them, so its mixed cell gets an image of its own."""
    shots = []

    def tie_cancel(img, cases, a, ini, mn):
        # two adjacent pixels at 200 (equal corners: NMS removes both at iniTh) and one pixel at 75 (score 14)
        x, y = a[0] + 6, a[1] + 6
        img[y, x] = 200; img[y, x + 1] = 200; img[y + 12, x + 10] = 75
        if ini != mn:
            cases.append(Case("tie-cancel cell: the weak corner appears on the retry and is kept", 0, (x + 10, y + 12), ("kp", 14, "retry_before_nms")))
        else:
            cases.append(Case("tie-cancel cell, iniTh == minTh: the weak corner is there at once", 0, (x + 10, y + 12), ("kp", 14)))
        cases.append(Case("tie-cancel cell: the pair is gone", 0, (x, y), ("no_cand",)))

    def sub_ini(img, cases, b, ini, mn):
        x, y = b[0] + 6, b[1] + 6
        (ax, ay), (bx, by) = RETRY_OFF
        img[y, x] = 75; img[y + ay, x + ax] = 68; img[y + by, x + bx] = 67                  # scores 14, 7, 6
        cases.append(Case("sub-iniTh cell: score 14", 0, (x, y), ("cand", 14)))
        cases.append(Case("sub-iniTh cell: score 7 == minTh", 0, (x + ax, y + ay), ("cand", 7, "score_gt")))
        cases.append(Case("sub-iniTh cell: score 6 < minTh", 0, (x + bx, y + by), ("no_cand",)))

    def mixed(img, cases, c, ini, mn):
        # one iniTh corner plus weaker ones, which must not appear
        x, y = c[0] + 6, c[1] + 6
        (ax, ay), (bx, by) = RETRY_OFF
        img[y, x] = 81; img[y + ay, x + ax] = 80; img[y + by, x + bx] = 68                  # scores 20, 19, 7
        cases.append(Case("mixed cell: score 20 == iniTh", 0, (x, y), ("cand", 20)))
        cases.append(Case("mixed cell: score 19 beside an iniTh corner", 0, (x + ax, y + ay), ("no_cand",) if ini == 20 else ("cand", 19)))
        cases.append(Case("mixed cell: score 7 beside an iniTh corner", 0, (x + bx, y + by), ("no_cand",) if ini == 20 else ("cand", 7)))

    # per canvas the images: (content, its cell, the empty cell that shares an edge with it), cells in row-major order
    layouts = {"staged": [[(tie_cancel, 0, 1), (mixed, 4, 3), (sub_ini, 14, 13)]],
               "generic": [[(tie_cancel, 0, 1), (sub_ini, 3, 2)], [(mixed, 1, 0), (mixed, 1, 3)]]}
    for cv in CANVASES:
        areas = scan_areas(cv.W, cv.H)
        for ini, mn in ((20, 7), (7, 7)):
            for k, layout in enumerate(layouts[cv.name]):
                img = np.full((cv.H, cv.W), 60, np.uint8); cases = []; filled = set()
                for fill, cell, free in layout:
                    if cell not in filled:                                                  # a cell with two free neighbours is filled once
                        fill(img, cases, areas[cell], ini, mn); filled.add(cell)
                        cases.append(Case("cell %d holds candidates" % cell, 0, None, ("cell_some", cell)))
                    cases.append(Case("cell %d, an edge neighbour of cell %d, holds no candidate" % (free, cell), 0, None, ("cell_count", free, 0)))
                shots.append(Shot("retry/%s/ini%d_min%d/%d" % (cv.name, ini, mn, k), img, params(cv, 500, ini, mn), cases))
    return shots


# ------------------------------------------------------------------------------------------------ lattice
def lattice_image(W, H, mod=8, mul=2, phase=0, bg=60, fg=200):
    """fg where (x + mul * y + phase) % mod == 0.  For (8, 2): no non-zero lattice vector lies on the 16-ring or in the 3 x 3
    neighbourhood, so every lattice pixel is an isolated corner of score fg - bg - 1 and nothing else is a corner."""
    y, x = np.mgrid[0:H, 0:W]
    return np.where((x + mul * y + phase) % mod == 0, fg, bg).astype(np.uint8)


LATTICE_COUNTS = {(640, 480): 33260, (331, 257): 7993, (200, 150): 2268}     # level-0 candidates (the issue's table)


def blank_to(img, target, count):
    """Blanks lattice pixels from the end of raster order until count(image) == target (count is monotone in the kept prefix)."""
    ys, xs = np.nonzero(img == 200)
    lo, hi = 0, len(ys)                                  # keep the first k lattice pixels
    while lo < hi:
        k = (lo + hi) // 2
        im = img.copy(); im[ys[k:], xs[k:]] = 60
        if count(im) < target:
            lo = k + 1
        else:
            hi = k
    im = img.copy(); im[ys[lo:], xs[lo:]] = 60
    assert count(im) == target, (count(im), target)
    return im


def lattice(count=None):
    """count(img) -> the oracle's cand_per_level[0] with one level (needed for the 2047 .. 8193 variants; None leaves them out)."""
    shots = []
    for (W, H), n in LATTICE_COUNTS.items():
        shots.append(Shot("lattice/%dx%d" % (W, H), lattice_image(W, H), (1000, 1.2, 1, 20, 7),
                          [Case("%d level-0 candidates, every response 139" % n, 0, None, ("ncand", n)),
                           Case("all responses tie: the first in candidate order wins every node", 0, None, ("twin", "tie_last"))]
                          + ([Case("more than 128 NMS survivors in one cell", 0, None, ("cell_over", 128))] if (W, H) != (640, 480) else [])))
    cv = GENERIC
    shots.append(Shot("lattice/generic", lattice_image(cv.W, cv.H), params(cv, 300, 20, 7),
                      [Case("more than 128 NMS survivors in one cell (generic kernel)", 0, None, ("cell_over", 128)),
                       Case("all responses tie", 0, None, ("twin", "tie_last"))]))
    if count is not None:
        for (W, H), targets in (((200, 150), (2047, 2048, 2049)), ((640, 480), (8191, 8192, 8193))):
            base = lattice_image(W, H)
            for t in targets:
                shots.append(Shot("lattice/%dx%d/M=%d" % (W, H, t), blank_to(base, t, lambda im: count(im, (1000, 1.2, 1, 20, 7))),
                                  (1000, 1.2, 1, 20, 7), [Case("exactly %d candidates: k_quadtree's switch point" % t, 0, None, ("ncand", t))]))
    return shots


# ------------------------------------------------------------------------------------------------ quadtree_edges
def quadtree_edges():
    """Sparse single-pixel corners with distinct responses around the quadtree's split lines.  200 x 150, one level: the key
    point area is 168 x 118, nIni = 1, the root splits at x = 84, y = 59 (node coordinates = level coordinates - 16), its first
    child at 42 / 30.  N = nfeatures (one level)."""
    cv = STAGED
    shots = []
    O = 16                                               # node coordinate 0 = level pixel 16

    def mk(name, nf, dots, claims, cv=cv):
        img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
        for (x, y, amp) in dots:
            img[y + O, x + O] = 60 + amp + 1
        for nm, (x, y), cl in claims:
            cases.append(Case(nm, 0, (x + O, y + O) if x is not None else None, cl))
        shots.append(Shot("quadtree_edges/" + name, img, params(cv, nf, 20, 7), cases))

    # first split, N = 2: after one pass there are 2 nodes (top left, top right) >= N.  The point ON the line goes right, where
    # it beats its weaker neighbour; one line further left it would beat the point left of it instead.
    mk("first split x", 2, [(83, 10, 100), (84, 20, 120), (85, 30, 110)],
       [("x = mid - 1: alone in the left node", (83, 10), ("kp", 100)), ("x = mid: goes right and wins there", (84, 20), ("kp", 120)),
        ("x = mid + 1: loses to the point on the line", (85, 30), ("no_kp",)), ("2 key points", (None, None), ("per_level", 2))])
    mk("first split y", 2, [(10, 58, 100), (20, 59, 120), (30, 60, 110)],
       [("y = mid - 1: alone in the top node", (10, 58), ("kp", 100)), ("y = mid: goes down and wins there", (20, 59), ("kp", 120)),
        ("y = mid + 1: loses to the point on the line", (30, 60), ("no_kp",))])
    # deeper split, N = 3: pass 1 gives 2 nodes (top left with 3 points, bottom right with 1); 2 + 3 > 3, so the sorted pass splits the
    # top-left node at x = 42 and reaches N at its end
    mk("deeper split x", 3, [(41, 8, 100), (42, 18, 120), (43, 28, 110), (150, 100, 90)],
       [("x = mid - 1 of the child", (41, 8), ("kp", 100)), ("x = mid of the child", (42, 18), ("kp", 120)),
        ("x = mid + 1 of the child", (43, 28), ("no_kp",)), ("the lone point", (150, 100), ("kp", 90)),
        ("N reached at the end of the sorted pass", (None, None), ("per_level", 3))])
    mk("deeper split y", 3, [(8, 29, 100), (18, 30, 120), (28, 31, 110), (150, 100, 90)],
       [("y = mid - 1 of the child", (8, 29), ("kp", 100)), ("y = mid of the child", (18, 30), ("kp", 120)),
        ("y = mid + 1 of the child", (28, 31), ("no_kp",))])
    # N reached exactly at the end of an unsorted pass: four populated quadrants, N = 4
    q4 = [(20, 20, 100), (30, 40, 90), (120, 20, 101), (140, 40, 91), (20, 80, 102), (50, 100, 92), (120, 80, 103), (150, 100, 93)]
    mk("N at the end of the unsorted pass", 4, q4,
       [("4 nodes == N after pass 1", (None, None), ("per_level", 4)), ("the weaker of a quadrant", (30, 40), ("no_kp",)),
        ("the stronger of a quadrant", (20, 20), ("kp", 100))])
    # N reached in the MIDDLE of the sorted pass: quadrants with 4, 3, 2, 1 points, N = 6.  4 + 3 * 3 > 6 -> sorted; the largest node (4 points
    # in 4 sub-quadrants) is split first: 3 + 4 = 7 >= 6 -> break; the nodes with 3 and 2 points stay whole and keep their best only
    mk("N in the middle of the sorted pass", 6,
       [(10, 10, 100), (60, 10, 101), (10, 45, 102), (60, 45, 103), (100, 10, 110), (130, 20, 111), (150, 40, 112), (20, 80, 120), (60, 100, 121),
        (140, 100, 130)],
       [("7 key points for N = 6", (None, None), ("per_level", 7)), ("the split node keeps all four", (10, 10), ("kp", 100)),
        ("the 3-point node was not split: its weakest is gone", (100, 10), ("no_kp",)), ("and its best stays", (150, 40), ("kp", 112)),
        ("the 2-point node was not split", (20, 80), ("no_kp",))])
    # the division ends when a pass adds no node: both points lie in the root's top-left child, 1 node before and after pass 1
    mk("a pass that adds no node", 500, [(10, 10, 100), (60, 40, 90)],
       [("two candidates", (None, None), ("ncand", 2)), ("one key point though the quota is 500", (None, None), ("per_level", 1)),
        ("the stronger of the undivided node", (10, 10), ("kp", 100)), ("the weaker is dropped", (60, 40), ("no_kp",))])
    # fewer candidates than the quota; exactly one candidate; none
    mk("fewer than the quota", 500, q4, [("all 8 candidates kept, quota 500", (None, None), ("per_level", 8))])
    mk("one candidate", 500, [(70, 50, 100)], [("exactly one candidate", (None, None), ("ncand", 1)), ("and it is kept", (70, 50), ("kp", 100))])
    # two levels at 2.0: a single pixel of score 21 is a corner on level 0 and averaged away on level 1
    cv2 = Canvas("staged2", 200, 150, 2.0, 2)
    mk("zero at a level", 500, [(70, 50, 21)], [("one candidate on level 0", (None, None), ("ncand", 1)), ("none on level 1", (None, None), ("ncand_level", (1, 0)))], cv=cv2)
    return shots


# ------------------------------------------------------------------------------------------------ small_quota
WIDE = (1241, 376)


def _synth():
    import __graft_entry__ as graft
    return graft.load_package().synth


def small_quota():
    """nfeatures 1 .. 50 on 8 levels of a wide image (nIni = 4 on level 0): quotas down to 0, below 4 * nIni on every level, and the
    quadtree still runs one full pass, so more key points than the quota come out (kpCap = max(quota + 3, 4 * nIni) + 1)."""
    W, H = WIDE
    shots = []
    for kind, img in (("lattice", lattice_image(W, H)), ("texture", _synth().random_image(W, H, 31, "texture"))):
        for nf in (1, 3, 8, 20, 50):
            shots.append(Shot("small_quota/%s/nf=%d" % (kind, nf), img, (nf, 1.2, 8, 20, 7),
                              [Case("more key points than the quota on some level", None, None, ("over_quota",)),
                               Case("more than 4 key points on level 0", 0, None, ("per_level_over", 4))]))
    return shots


# ------------------------------------------------------------------------------------------------ orientation
ORI = Canvas("ori", 240, 160, 1.2, 1)                   # 6 x 4 cells of 35 x 32: one level, patches 40 px apart
PATCH_SUM_U = sum(u for v in range(-15, 16) for u in range(1, UMAX[abs(v)] + 1))    # sum of u over the right half of the circular patch


def set_moments(img, cx, cy, m01, m10, amp=4):
    """Raises pixels of row v = 0 and column u = 0 of the patch (not the centre, not the ring's compass points) by at most `amp`,
    so that the patch's moments change by exactly (m01, m10).  Raised by less than minThFAST they cannot become corners."""
    for m, horizontal in ((m10, True), (m01, False)):
        rem, sg = abs(m), (1 if m >= 0 else -1)
        for u in [k for k in range(15, 0, -1) if k != 3]:
            d = min(amp, rem // u)
            rem -= d * u
            if d:
                if horizontal:
                    img[cy, cx + sg * u] += d
                else:
                    img[cy + sg * u, cx] += d
        assert rem == 0, "moment %d is not reachable with amplitude %d" % (m, amp)


def patch_centres(cv, pitch=40, first=36):
    return [(x, y) for y in range(first, cv.H - first + 1, pitch) for x in range(first, cv.W - first + 1, pitch)]


def orientation():
    """One isolated corner (a single pixel, +140) per 31-px patch with its moments set exactly; key points on the extractor's
    border limits; and the half-plane patch with m01 = -1 against the largest m10 a patch can hold."""
    cv = ORI
    shots = []
    L = 400
    ms = [(0, 0), (1, L), (-1, L), (1, -L), (-1, -L), (L, 1), (L, -1), (-L, 1), (-L, -1), (0, 1), (0, -1), (1, 0), (-1, 0), (0, L), (L, 0),
          (5, 5), (5, -5), (-5, 5), (-5, -5), (L, L), (L, -L), (-L, L), (-L, -L), (1, 1), (-1, -1), (L, L - 1), (L - 1, L), (-L, L - 1), (L - 1, -L), (0, -L)]
    cen = patch_centres(cv)
    for i0 in range(0, len(ms), len(cen)):
        img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
        for (m01, m10), (cx, cy) in zip(ms[i0:i0 + len(cen)], cen):
            img[cy, cx] = 200
            set_moments(img, cx, cy, m01, m10)
            cases.append(Case("moments m01=%d m10=%d" % (m01, m10), 0, (cx, cy), ("moments", (m01, m10))))
        shots.append(Shot("orientation/moments/%d" % (i0 // len(cen)), img, params(cv, 500, 20, 7), cases))
    # on the border limits: first / last scanned column and row of the level (x = 19, W - 20; y = 19, H - 20) and two image corners
    img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
    for nm, (x, y) in (("left", (19, 60)), ("right", (cv.W - 20, 100)), ("top", (90, 19)), ("bottom", (150, cv.H - 20)),
                       ("top left", (19, 19)), ("bottom right", (cv.W - 20, cv.H - 20)), ("middle", (120, 80))):
        img[y, x] = 200
        set_moments(img, x, y, 7, -3) if nm == "middle" else None
        cases.append(Case("key point on the %s limit" % nm, 0, (x, y), ("kp", 139)))
    shots.append(Shot("orientation/limits", img, params(cv, 500, 20, 7), cases))
    # half plane: 0 left of and on the centre column, 255 right of it; centre 100 (9 ring pixels at 0: score 99); the pixel above the
    # centre at 1 -> m01 = -1, m10 = 255 * sum(u > 0): the steepest angle below 360 degrees this patch geometry holds
    img = np.zeros((cv.H, cv.W), np.uint8)
    cx, cy = 120, 80
    img[:, cx + 1:] = 255; img[cy, cx] = 100; img[cy - 1, cx] = 1
    shots.append(Shot("orientation/half_plane", img, params(cv, 500, 20, 7),
                      [Case("m01 = -1 against the largest m10", 0, (cx, cy), ("moments", (-1, 255 * PATCH_SUM_U))),
                       Case("angle just below 360", 0, (cx, cy), ("angle_in", (359.99, 360.0)))]))
    return shots


# ------------------------------------------------------------------------------------------------ descriptor
def reach(angle):
    t, _ = tap_coords(angle)
    return int(np.abs(t).max())


# Found by scanning every (m01, m10) in [-250, 250]^2 with the oracle's fastAtan2 and its own a, b (152 192 distinct angles): the only
# five at which a pattern coordinate x * a - y * b or x * b + y * a lands EXACTLY on k + .5 with k even (half-to-even and half-away
# then pick different pixels; at odd k both give k + 1), and the first angle whose rounded pattern reaches 18 px = SD_DP_R.
TIE_MOMENTS = [(-157, -6), (-157, 6), (-131, 205), (28, -129), (232, -83)]
FAR_MOMENTS = (-120, -119)


def sym_noise_patch(img, cx, cy, seed, amp=6, r=19):
    """bg + point-symmetric noise 0 .. amp: zero moments, no two halves alike, and (amp < minThFAST) no corner."""
    side = 2 * r + 1
    n = np.random.default_rng(seed).integers(0, amp + 1, side * side)
    n[side * side // 2 + 1:] = n[:side * side // 2][::-1]                     # the second half of raster order = the first, through the centre
    n = n.reshape(side, side)
    assert np.array_equal(n, n[::-1, ::-1])
    img[cy - r:cy + r + 1, cx - r:cx + r + 1] = 60 + n


def descriptor(fast_atan2=None, blur=None):
    """fast_atan2(m01, m10) and blur(img) are the oracle's leaves (needed for the searched cases; None leaves those out)."""
    cv = ORI
    shots = []
    # flat: a pixel 8 above the background is a corner of score 7 == minTh, and the 7 x 7 blur rounds it away: every tap ties
    img = np.full((cv.H, cv.W), 60, np.uint8)
    img[80, 120] = 68; img[40, 60] = 68; img[120, 180] = 52
    shots.append(Shot("descriptor/flat", img, params(cv, 500, 20, 7),
                      [Case("blurred patch flat: all 256 taps tie, descriptor zero", 0, (120, 80), ("desc_zero", "desc_le")),
                       Case("the same, darker than the background", 0, (180, 120), ("desc_zero", "desc_le"))]))
    # two grey values: 8-px squares of 200 on 60, 16 px apart
    y, x = np.mgrid[0:cv.H, 0:cv.W]
    img = np.where((x % 16 < 8) & (y % 16 < 8), 200, 60).astype(np.uint8)
    shots.append(Shot("descriptor/two_greys", img, params(cv, 500, 20, 7),
                      [Case("two grey values: taps inside one block tie", None, None, ("twin_desc", "desc_le"))]))
    if fast_atan2 is None:
        return shots
    # rounding: a tap exactly on .5.  Each patch is point-symmetric noise of amplitude 6 (zero moments) plus set_moments; of the seeds
    # the first whose descriptor changes under round-half-away is kept (deterministic: the oracle's own blur decides)
    img = np.full((cv.H, cv.W), 60, np.uint8); cases = []
    cen = patch_centres(cv, pitch=48, first=40)
    for (m01, m10), (cx, cy) in zip(TIE_MOMENTS + [FAR_MOMENTS], cen):
        ang = fast_atan2(m01, m10)
        for seed in range(64):
            trial = img.copy()
            sym_noise_patch(trial, cx, cy, seed)
            trial[cy, cx] = 230
            set_moments(trial, cx, cy, m01, m10)
            if (m01, m10) == FAR_MOMENTS:
                break
            b = blur(trial)
            if not np.array_equal(describe(b, cx, cy, ang), describe(b, cx, cy, ang, "round_away")):
                break
        img = trial
        if (m01, m10) == FAR_MOMENTS:
            cases.append(Case("rounded pattern reaches 18 px = the rim of the staged patch, angle %r" % ang, 0, (cx, cy), ("reach", 18, (m01, m10))))
        else:
            cases.append(Case("a tap exactly on .5 at angle %r (m01=%d m10=%d, noise seed %d)" % (ang, m01, m10, seed), 0, (cx, cy),
                              ("desc_tie", (m01, m10), "round_away")))
    shots.append(Shot("descriptor/searched", img, params(cv, 500, 20, 12), cases))
    return shots


# ------------------------------------------------------------------------------------------------ planes
def plane_contents(W, H, seed):
    y, x = np.mgrid[0:H, 0:W]
    tex = _synth().random_image(W, H, seed, "texture").copy()
    sat = tex.copy(); sat[H // 4:H // 2 + 9, W // 5:W // 2 + 7] = 255
    return [("zeros", np.zeros((H, W), np.uint8), True), ("ones", np.full((H, W), 255, np.uint8), True),
            ("saturated block", sat, False), ("checkerboard", (((x + y) & 1) * 255).astype(np.uint8), None),
            ("ramp x", (x * 255 // (W - 1)).astype(np.uint8), None), ("ramp y", (y * 255 // (H - 1)).astype(np.uint8), None),
            ("texture", tex, False)]


# Per (W, H, scale factor): for every level >= 1 the tile grid (tilesX, tilesY) of k_pyr_level_tiles over that level's padded plane and
# whether the level runs that kernel (True) or the per-thread k_pyr_level (False).  Worked out from the plan by hand, witnessed by
# pyr_paths().  k_pyr_level_tiles writes levels >= 1 only, so a tile edge is met by a LEVEL-1 plane: its padded width + 5 (the tiles start
# 5 px left of the plane) on 255 / 256 / 257 and its padded height on 207 / 208 / 209 come from level 0 = 255 x 203, 256 x 204, 257 x 205 at
# 1.2 and 425 x 338, 426 x 340, 427 x 342 at 2.0: one tile column filled to its last but one and to its last pixel, then a second column
# that holds one pixel; 13 tile rows, the last with 15 and 16 rows, then a 14th with one.  The first three sizes put the LEVEL-0 padded
# plane on 255 .. 257 x 207 .. 209 (k_pyr_level0's rows), the next three the width on 127 .. 129 (k_blur_wide's 128-px tile).
PLANE_PATHS = {
    (217, 169, 1.2): [(1, 12, True), (1, 10, True)], (217, 169, 2.0): [(1, 8, True)],
    (218, 170, 1.2): [(1, 12, True), (1, 10, True)], (218, 170, 2.0): [(1, 8, True)],
    (219, 171, 1.2): [(1, 12, True), (1, 10, True)], (219, 171, 2.0): [(1, 8, True)],
    (127, 130, 1.2): [(1, 10, True), (1, 8, True)], (127, 130, 2.0): [(1, 7, True)],
    (128, 130, 1.2): [(1, 10, True), (1, 8, True)], (128, 130, 2.0): [(1, 7, True)],
    (129, 130, 1.2): [(1, 10, True), (1, 8, True)], (129, 130, 2.0): [(1, 7, True)],
    (255, 203, 1.2): [(1, 13, True), (1, 12, True)], (256, 204, 1.2): [(1, 13, True), (1, 12, True)], (257, 205, 1.2): [(2, 14, True), (1, 12, True)],
    (425, 338, 2.0): [(1, 13, True)], (426, 340, 2.0): [(1, 13, True)], (427, 342, 2.0): [(2, 14, True)],
    # ratio 2.5: 256 x 16 tile pixels read 640 x 40 source pixels, 40 * (656 + 512) = 46,720 B of LDS: still the tile kernel.  Ratio 3: 50 source
    # rows of at least 640 + 16 + 512 B are more than 48 KiB: the per-thread kernel, with one and with two tile columns' worth of width
    (1241, 376, 2.5): [(3, 12, True)], (1241, 376, 3.0): [(2, 11, False)], (600, 200, 3.0): [(1, 7, False)]}
PLANE_SIZES = [(217, 169), (218, 170), (219, 171), (127, 130), (128, 130), (129, 130)]
PLANE_EDGES = {1.2: [(255, 203), (256, 204), (257, 205)], 2.0: [(425, 338), (426, 340), (427, 342)]}
PLANE_LEVEL1 = {(255, 203): (255, 207), (256, 204): (256, 208), (257, 205): (257, 209),       # level 1's padded width + 5, padded height
                (425, 338): (255, 207), (426, 340): (256, 208), (427, 342): (257, 209)}


def plane_cases(W, H, scale, nm, empty):
    """What a plane shot claims: its content's outcome and the pyramid kernel of every level."""
    if empty is None and nm == "checkerboard":
        # no ring of a 1-px checkerboard holds 9 contiguous pixels of one value; resampled at 1.2 it beats into a moire with corners, at 2 and more
        # every output pixel averages as many black as white source pixels
        content = [Case("checkerboard: no corner on level 0", 0, None, ("ncand", 0)),
                   Case("checkerboard: moire corners above", None, None, ("has_kp",))] if scale == 1.2 else [Case("checkerboard averaged flat", None, None, ("empty",))]
    elif empty is None:
        # a plane that is monotone along one axis and constant across it has no corner: only 7 contiguous ring pixels lie strictly on one side
        # (the resized levels are constant across to one grey value, far below minTh)
        content = [Case(nm + ": no corner, every level's plane monotone along the ramp and constant across it to one grey value", None, None, ("ramp", nm[-1]))]
    else:
        content = [Case(nm, None, None, ("empty",) if empty else ("has_kp",))]
    path = PLANE_PATHS[(W, H, scale)]
    what = ", ".join("level %d %s (%d x %d tiles)" % (l + 1, "k_pyr_level_tiles" if t else "k_pyr_level", tx, ty) for l, (tx, ty, t) in enumerate(path))
    cases = content + [Case("pyramid kernels: " + what, None, None, ("pyr_path", tuple(path)))]
    if (W, H) in PLANE_LEVEL1:
        cases.append(Case("level 1's padded plane + 5 is %d wide and %d high" % PLANE_LEVEL1[(W, H)], 1, None, ("tile_edge", PLANE_LEVEL1[(W, H)])))
    return cases


def planes():
    """Pyramid and blur planes around the row length of k_pyr_level0, the tile of k_pyr_level_tiles (256 x 16 over a level >= 1's padded
    plane, 5 px to its left) and k_blur_wide's (128 wide), at scale factors 1.2 and 2.0; 2.5 on the wide image (still the tile kernel) and
    3.0 on it and on 600 x 200 (the per-thread k_pyr_level)."""
    shots = []
    for scale, nl in ((1.2, 3), (2.0, 2)):
        for W, H in PLANE_SIZES + PLANE_EDGES[scale]:
            for nm, img, empty in plane_contents(W, H, 40 + W):
                shots.append(Shot("planes/%dx%d/%.1f/%s" % (W, H, scale, nm), img, (300, scale, nl, 20, 7), plane_cases(W, H, scale, nm, empty)))
    for (W, H), scale, first in ((WIDE, 2.5, 4), (WIDE, 3.0, 4), ((600, 200), 3.0, 2)):
        for nm, img, empty in plane_contents(W, H, 47)[first:]:
            shots.append(Shot("planes/%dx%d/%.1f/%s" % (W, H, scale, nm), img, (300, scale, 2, 20, 7), plane_cases(W, H, scale, nm, empty)))
    return shots


FUZZ_SEED, FUZZ_DRAWS = 29, 8                          # the crafted draws of tools/fuzz_extract.py that the tests run


BUILDERS = ("threshold_edges", "nms_ties", "retry", "lattice", "quadtree_edges", "small_quota", "orientation", "descriptor", "planes")


def build_all(orc):
    """Every builder's shots, the searched ones with the oracle's leaves: {builder: [Shot]}."""
    def count(im, prm):
        o = orc.Extractor(*prm); o(im)
        return int(o.cand_per_level[0])
    out = {}
    for b in BUILDERS:
        f = globals()[b]
        if b == "lattice":
            out[b] = f(count)
        elif b == "descriptor":
            out[b] = f(orc.fast_atan2, orc.gaussian7)
        else:
            out[b] = f()
    return out
