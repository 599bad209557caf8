"""Shared by test_oracle_cull.py, test_gpu_cull.py and tools/fuzz_cull.py: seeded cases with CRAFTED key points, descriptors,
boxes and models for the dynamic-object cull (k_box_separate / k_separate / k_update_frame, csrc/k_cull.h).  Plain numpy.

A case is a pair of frames (reference, current): per frame key points (KP_DTYPE, class_id -1, octave 0, positions inside the
image), 32-byte descriptors, boxes (f64 x, y, w, h) and their ids; a model M (3 x 3 f32) with flag 1 (H) or 2 (F); the last frame's
ids and statuses; a name.  Descriptors force the intended matches: random base descriptors (mutual distance >= 60) and partners
that are a copy with a chosen number of flipped bits.  A case's seed depends on its kind and parameters only, never on its place
in a list, so the CPU tests that say which branch a case reaches and the GPU tests that run it speak of the same arrays.

Domain (check_domain): class_id == -1 on entry.  Frame::firstSeparate keeps a class id that is already set where k_box_separate
overwrites it with the original index; no frame reaches the cull that way (the extractor writes -1 and firstSeparate runs once
per frame), so such input is outside the domain.  A frame without key points has no boxes either: the constructor returns before
boxTrack (Frame.cc:160-161, 320-321), so the oracle side drops the boxes of an empty frame as the kernel does."""
import itertools

import numpy as np

import stereo_cases as sc

KP_DTYPE = sc.KP_DTYPE
F32 = np.float32
SEED = 33
MAXB = 64
TH_H, TH_F = 5.991, 5.841
GEOM = sc.GEOMS["752x240-8x1.2"]
# the only group that needs more than SD_BF_TCAP = 2048 key points in one box
GEOM_BIG = sc.Geom("752x240-8x1.2-4300", 752, 240, 8, 1.2, 435.2046959714599, 47.90639384423901, n_features=4300)
W, H = GEOM.W, GEOM.H
I3 = np.eye(3, dtype=F32)
EPI = (376.0, -2000.0)                      # epipole far above the image: the epipolar lines are steep, their normals close to x
H_GENERAL = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
# Camera.k1 .. k3 of Examples/RGB-D/TUM1.yaml on this geometry's intrinsics
DIST_K4 = np.array([435.2047, 435.2047, 376.0, 120.0], F32)
DIST_D5 = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], F32)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def cross(e):
    return np.array([[0, -1.0, e[1]], [1.0, 0, -e[0]], [-e[1], e[0], 0]])


F_IDENT = cross(EPI).astype(F32)            # F = [e]x I: p2 == p1 lies on its epipolar line; every entry is an f32 value


# ---- descriptors
def hamming_matrix(a, b):
    """(len(a), len(b)) Hamming distances; exact (sums of at most 256 ones in f32)."""
    A = np.unpackbits(np.asarray(a, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    B = np.unpackbits(np.asarray(b, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return (A @ (1 - B).T + (1 - A) @ B.T).astype(np.int32)


def bases(rng, n):
    """n random descriptors at mutual distance >= 60."""
    d = sc.rand_desc(rng, n)
    if n > 1:
        D = hamming_matrix(d, d) + 256 * np.eye(n, dtype=np.int32)
        assert D.min() >= 60, "base descriptors too close (%d)" % D.min()
    return d


def kps(x, y):
    return sc.kps(GEOM, x, y, 0)


def steps(x, k):
    """The f32 value k representable steps above the positive f32 x."""
    return (np.asarray(x, F32).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(F32)


# ---- frames and cases
def frame(kp=None, desc=None, boxes=(), ids=()):
    kp = np.zeros(0, KP_DTYPE) if kp is None else np.ascontiguousarray(kp, KP_DTYPE)
    desc = np.zeros((0, 32), np.uint8) if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return dict(kp=kp, desc=desc, boxes=np.asarray(boxes, np.float64).reshape(-1, 4), ids=np.asarray(ids, np.int32).reshape(-1))


def case(name, ref, cur, M=I3, flag=1, last_idx=(), last_status=(), dist=False, cap=None, **info):
    c = dict(name=name, kind=name.split("-")[0], ref=ref, cur=cur, M=np.ascontiguousarray(M, F32).reshape(3, 3), flag=int(flag),
             last_idx=np.asarray(last_idx, np.int32).reshape(-1), last_status=np.asarray(last_status, np.int32).reshape(-1), dist=dist)
    c.update(info)
    return check_domain(c, cap)


def check_domain(c, cap=None):
    cap = GEOM.cap if cap is None else cap
    assert c["flag"] in (1, 2) and c["M"].dtype == F32 and c["M"].shape == (3, 3), c["name"]
    assert len(c["last_idx"]) == len(c["last_status"]) <= MAXB, c["name"]
    for f in (c["ref"], c["cur"]):
        k, d = f["kp"], f["desc"]
        assert k.dtype == KP_DTYPE and d.dtype == np.uint8 and d.shape == (len(k), 32), c["name"]
        assert len(k) <= cap, "%s: %d key points, capacity %d" % (c["name"], len(k), cap)
        assert (k["class_id"] == -1).all() and (k["octave"] == 0).all(), c["name"]
        assert ((k["x"] >= 0) & (k["x"] < W) & (k["y"] >= 0) & (k["y"] < H)).all(), "%s: key point outside the image" % c["name"]
        assert f["boxes"].dtype == np.float64 and f["boxes"].shape == (len(f["ids"]), 4) and len(f["ids"]) <= MAXB, c["name"]
        assert np.isfinite(f["boxes"]).all(), c["name"]
        assert np_membership(k, f["boxes"]).sum() <= 2 * cap, "%s: more box items than the item table holds" % c["name"]
    return c


class Pair:
    """Builds the two frames of a case box by box.  Tiles of 94 x 60 pixels (8 x 3 of them, rows 0 .. 179) keep boxes apart; the rows
    from 184 down hold the static key points."""

    def __init__(self, name, *key):
        self.name, self.rng = name, _rng(*key)
        self.k = [[], []]; self.d = [[], []]; self.b = [[], []]; self.i = [[], []]

    @staticmethod
    def tile_rect(t):
        return (94.0 * (t % 8) + 2.0, 60.0 * (t // 8) + 2.0, 90.0, 56.0)

    def points(self, n, t):
        x0, y0 = 94.0 * (t % 8), 60.0 * (t // 8)
        return self.rng.uniform(x0 + 6, x0 + 76, n), self.rng.uniform(y0 + 6, y0 + 54, n)

    def add(self, side, kp, desc):
        self.k[side].append(kp); self.d[side].append(np.asarray(desc, np.uint8).reshape(-1, 32))

    def add_box(self, side, rect, id_):
        self.b[side].append(rect); self.i[side].append(id_)

    def matched(self, t, n, dyn=(), flips=(0, 12), n_ref_extra=0, n_cur_extra=0):
        """n intended pairs in tile t: the current key point on its partner's place, or 10 px to its right for the indices in dyn;
        then unpartnered key points with descriptors of their own.  -> (kr, dr, kc, dc)"""
        rng = self.rng
        x, y = self.points(n + n_ref_extra, t)
        base = bases(rng, n + n_ref_extra + n_cur_extra)
        kr, dr = kps(x, y), base[:n + n_ref_extra]
        off = np.zeros(n); off[list(dyn)] = 10.0
        xe, ye = self.points(n_cur_extra, t)
        kc = kps(np.concatenate([x[:n] + off, xe]), np.concatenate([y[:n], ye]))
        dc = np.concatenate([sc.flipped(rng, base[:n], rng.integers(flips[0], flips[1] + 1, n)) if n else base[:0], base[n + n_ref_extra:]])
        return kr, dr, kc, dc

    def box(self, t, id_, n, ref_id=None, **kw):
        """A box on tile t in both frames with n intended pairs."""
        kr, dr, kc, dc = self.matched(t, n, **kw)
        self.add(0, kr, dr); self.add(1, kc, dc)
        self.add_box(0, self.tile_rect(t), id_ if ref_id is None else ref_id); self.add_box(1, self.tile_rect(t), id_)
        return self

    def statics(self, n):
        for side in (0, 1):
            self.add(side, kps(self.rng.uniform(4, W - 4, n), self.rng.uniform(186, H - 2, n)), bases(self.rng, n))
        return self

    def frames(self):
        out = []
        for s in (0, 1):
            k = np.concatenate(self.k[s]) if self.k[s] else None
            d = np.concatenate(self.d[s]) if self.d[s] else None
            out.append(frame(k, d, self.b[s], self.i[s]))
        return out

    def case(self, **kw):
        ref, cur = self.frames()
        return case(self.name, ref, cur, **kw)


# ---- independent numpy restatements (the CPU tests compare the oracle with these)
def np_membership(kp, boxes):
    """(N, nb) bool: cv::Rect2d::contains on the f32 position widened to f64 (left / top inclusive, right / bottom exclusive)."""
    px = kp["x"].astype(np.float64)[:, None]; py = kp["y"].astype(np.float64)[:, None]
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return (b[:, 0] <= px) & (px < b[:, 0] + b[:, 2]) & (b[:, 1] <= py) & (py < b[:, 1] + b[:, 3])


def erase_walk(has):
    """Original indices of the boxes that survive Frame.cc:585-592 (the loop index advances after an erase; hasKpts is not erased)."""
    kept = list(range(len(has)))
    i = 0
    while i < len(kept):
        if not has[i]:
            del kept[i]
        i += 1
    return kept


def np_first_separate(f):
    """Box lists of a frame as the reference builds them: (kept_orig, lists) with lists[b] = ORIGINAL key-point indices."""
    m = np_membership(f["kp"], f["boxes"])
    if len(f["kp"]) == 0:
        return [], []
    has = m.any(0)
    kept = erase_walk(has)
    lists = [[] for _ in kept]
    empty = not has.all()
    for j in range(m.shape[1]):
        if not has[j]:
            continue
        bj = j - int((~has[:j + 1]).sum()) if empty else j
        if 0 <= bj < len(kept):
            lists[bj] = np.nonzero(m[:, j])[0].tolist()
    return kept, lists


def np_crosscheck(q, t):
    """cv::BFMatcher(NORM_HAMMING, crossCheck = true): first nearest wins both ways.  -> (n, 2) (query, train), (nq, nt) distances"""
    D = hamming_matrix(q, t)
    fwd, bwd = D.argmin(1), D.argmin(0)
    i = np.arange(len(q))
    ok = bwd[fwd] == i
    return np.stack([i[ok], fwd[ok]], 1).astype(np.int32), D


def chi2_f64(M, flag, p1, p2):
    """Plain float64 classifyH / classifyF: (chi2 of p1 against p2's transfer, chi2 of p2 against p1's transfer); p1 in the
    reference frame, p2 in the current one, (n, 2) each.  H: np.linalg.inv; F: point-to-line distances."""
    M = np.asarray(M, np.float64)
    P1 = np.concatenate([np.asarray(p1, np.float64), np.ones((len(p1), 1))], 1)
    P2 = np.concatenate([np.asarray(p2, np.float64), np.ones((len(p2), 1))], 1)
    with np.errstate(all="ignore"):
        if flag == 1:
            try:
                Mi = np.linalg.inv(M)
            except np.linalg.LinAlgError:
                Mi = np.full((3, 3), np.nan)
            a = P2 @ Mi.T; b = P1 @ M.T
            c1 = ((P1[:, :2] - a[:, :2] / a[:, 2:]) ** 2).sum(1)
            c2 = ((P2[:, :2] - b[:, :2] / b[:, 2:]) ** 2).sum(1)
        else:
            l2 = P1 @ M.T                      # line of p1 in the current image
            l1 = P2 @ M                        # line of p2 in the reference image
            c1 = (l2 * P2).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
            c2 = (l1 * P1).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return c1, c2


# ---- generators
def membership_edges():
    out = []
    # (a) key points on the four limits of boxes whose coordinates are / are not f32 values
    P = Pair("membership_edges-limits", 1, 0)
    rects = [(100.1, 0.1 + 0.2, 50.3, 40.7), (300.0, 60.0, 50.0, 40.0), (500.3, 100.7, 0.1 + 0.2, 20.1)]
    for side in (0, 1):
        for bi, (x, y, w, h) in enumerate(rects):
            xs, ys = [], []
            for lim in (x, x + w):
                hi = F32(lim) if np.float64(F32(lim)) >= lim else np.nextafter(F32(lim), F32(np.inf))      # first f32 >= the limit
                xs += [hi, np.nextafter(hi, F32(-np.inf))]; ys += [F32(y + h / 2)] * 2
            for lim in (y, y + h):
                hi = F32(lim) if np.float64(F32(lim)) >= lim else np.nextafter(F32(lim), F32(np.inf))
                ys += [hi, np.nextafter(hi, F32(-np.inf))]; xs += [F32(x + w / 2)] * 2
            n = len(xs)
            P.add(side, kps(np.array(xs, F32), np.array(ys, F32)), bases(_rng(1, 1, bi), n) if side == 0 else sc.flipped(P.rng, bases(_rng(1, 1, bi), n), 5))
            P.add_box(side, (x, y, w, h), 40 + bi)
    out.append(P.statics(6).case(limits=rects))
    # (b) empty and misplaced rectangles next to a populated box
    P = Pair("membership_edges-degenerate", 1, 2).box(9, 5, 6).statics(5)
    x0, y0 = 94.0 * 3 + 10, 60.0 + 10                       # tile 11: key points that no box may claim
    for side in (0, 1):
        P.add(side, kps(np.array([x0, x0 + 5, x0 + 10], F32), np.array([y0, y0 + 5, y0 + 10], F32)), bases(_rng(1, 3, side), 3))
        for j, r in enumerate([(x0 - 5, y0 - 5, 0.0, 30.0), (x0 + 30, y0 - 5, -40.0, 30.0), (x0 - 5, y0 + 30, 40.0, -40.0),
                               (800.0, 300.0, 50.0, 50.0), (-100.0, -80.0, 50.0, 60.0), (-1e9, 10.0, 10.0, 10.0)]):
            P.add_box(side, r, 60 + j)
    out.append(P.case())
    # (c) a box that covers the whole image: every key point is dynamic
    P = Pair("membership_edges-whole", 1, 4)
    kr, dr, kc, dc = P.matched(4, 12)
    for side, (k, d) in enumerate(((kr, dr), (kc, dc))):
        k["x"][0] = 0.0; k["y"][0] = 0.0; k["x"][1] = np.nextafter(F32(W), F32(0)); k["y"][1] = np.nextafter(F32(H), F32(0))
        P.add(side, k, d); P.add_box(side, (0.0, 0.0, float(W), float(H)), 3)
    out.append(P.case())
    # (d) a key point inside 1, 2, 3 and 64 boxes
    P = Pair("membership_edges-depth", 1, 5).statics(30)
    x = np.array([150, 160, 250, 260, 350, 360, 620, 630], np.float64); y = np.array([20, 30, 40, 50, 60, 70, 110, 120], np.float64)
    b = bases(P.rng, 8)
    P.add(0, kps(x, y), b); P.add(1, kps(x, y), sc.flipped(P.rng, b, 6))
    for side in (0, 1):
        for j in range(64):
            P.add_box(side, ((100.0, 200.0, 300.0)[j] if j < 3 else 600.0, 5.0, (540.0, 440.0, 340.0)[j] if j < 3 else 40.0, 130.0), 100 + j)
    out.append(P.case())
    # (e) 64 boxes, only box 63 (bit 63 of the mask) populated
    P = Pair("membership_edges-bit63", 1, 6).statics(4)
    kr, dr, kc, dc = P.matched(10, 8)
    P.add(0, kr, dr); P.add(1, kc, dc)
    for side in (0, 1):
        for j in range(63):
            P.add_box(side, (4.0 + 10 * j, 150.0, 3.0, 3.0), 200 + j)
        P.add_box(side, P.tile_rect(10), 263)
    out.append(P.case())
    return out


def empty_box_patterns():
    """Every pattern of populated / empty boxes for nb = 1 .. 6 in both frames (126 cases; the name carries the pattern, box 0 first),
    nb = 0, and a frame without key points that is given boxes (either side)."""
    out = []
    for nb in range(1, 7):
        for bits in itertools.product((0, 1), repeat=nb):
            P = Pair("empty_box_patterns-%s" % "".join(map(str, bits)), 2, nb, int("1" + "".join(map(str, bits)), 2)).statics(2)
            for j, on in enumerate(bits):
                if on:
                    P.box(j, 20 + j, 3)
                else:
                    for side in (0, 1):
                        P.add_box(side, (94.0 * j + 40, 100.0 + j, 1.0 + j, 1.0), 20 + j)
            out.append(P.case(pattern=bits, last_idx=[20, 21, 22], last_status=[0, 1, 2]))
    out.append(Pair("empty_box_patterns-none", 2, 0).statics(9).case(pattern=()))
    for side in (0, 1):
        P = Pair("empty_box_patterns-no_keypoints_%s" % ("ref", "cur")[side], 2, 7, side).box(1, 4, 5).box(2, 5, 5).statics(3)
        fr = P.frames()
        fr[side] = frame(None, None, fr[side]["boxes"], fr[side]["ids"])
        out.append(case(P.name, fr[0], fr[1], pattern=None))
    return out


PARTITION_SIZES = (1, 255, 256, 257, 511, 513)


def _partition(name, N, dyn, key):
    """N key points, those with dyn[i] inside the one box (rows 0 .. 119), the others below it; the same layout in both frames."""
    rng = _rng(3, *key)
    dyn = np.asarray(dyn, bool)
    x = rng.uniform(4, W - 16, N); y = np.where(dyn, rng.uniform(2, 118, N), rng.uniform(122, H - 2, N))
    d = sc.rand_desc(rng, N)
    ref = frame(kps(x, y), d, [(0.0, 0.0, float(W), 120.0)], [1])
    cur = frame(kps(x, y), sc.flipped(rng, d, 4), [(0.0, 0.0, float(W), 120.0)], [1])
    return case(name, ref, cur)


def partition_sizes(cap=None):
    cap = GEOM.cap if cap is None else cap
    out = []
    for N in PARTITION_SIZES + (cap,):
        dyn = np.arange(N) % 2 == 0
        dyn[0] = dyn[-1] = True
        out.append(_partition("partition_sizes-n%d-alternating" % N, N, dyn, (N, 0)))
    for N in (257, cap):
        out.append(_partition("partition_sizes-n%d-static" % N, N, np.zeros(N, bool), (N, 1)))
        out.append(_partition("partition_sizes-n%d-dynamic" % N, N, np.ones(N, bool), (N, 2)))
    st = np.ones(300, bool); st[0] = st[-1] = False
    out.append(_partition("partition_sizes-n300-static_ends", 300, st, (300, 3)))
    return out


MATCH_SIZES = ((1, 1), (1, 257), (257, 1), (257, 257), (2, 2), (3, 255), (255, 256), (256, 255), (256, 257), (257, 2), (2, 256), (255, 1))


def match_sizes():
    out = []
    for nq, nt in MATCH_SIZES:
        n = min(nq, nt)
        out.append(Pair("match_sizes-%dx%d" % (nq, nt), 4, nq, nt).box(5, 9, n, n_ref_extra=nt - n, n_cur_extra=nq - n).statics(3).case(sizes=(nq, nt)))
    return out


def _tie_case(name, key, n, edit):
    """One box of n pairs whose descriptors `edit(rng, dr, dc)` then rewrites; a second ordinary box follows."""
    P = Pair(name, 5, *key)
    kr, dr, kc, dc = P.matched(3, n, flips=(4, 12))
    edit(P.rng, kr, dr, kc, dc)
    P.add(0, kr, dr); P.add(1, kc, dc)
    for side in (0, 1):
        P.add_box(side, P.tile_rect(3), 11)
    return P.box(12, 12, 5).statics(3).case()


def hamming_ties():
    out = []

    def two_trains(rng, kr, dr, kc, dc):
        dr[2] = sc.flipped(rng, dc[4:5], 20)[0]; dr[5] = sc.flipped(rng, dc[4:5], 20)[0]; dr[4] = bases(rng, 1)[0]      # query 4: trains 2 and 5 at 20 bits
        dc[2] = bases(rng, 1)[0]; dc[5] = bases(rng, 1)[0]
        dc[7] = sc.flipped(rng, dr[6:7], 30)[0]                                                                         # query 7's nearest train 6 prefers query 6
        dr[7] = bases(rng, 1)[0]
        kc["x"][4] = kr["x"][2]; kc["y"][4] = kr["y"][2]                                                                # the match (4, 2) is on the spot
    out.append(_tie_case("hamming_ties-two_trains_and_cross_check", (0,), 10, two_trains))
    for a, b in ((3, 4), (255, 256), (3, 259)):
        def two_queries(rng, kr, dr, kc, dc, a=a, b=b):
            dc[a] = sc.flipped(rng, dr[a:a + 1], 20)[0]; dc[b] = sc.flipped(rng, dr[a:a + 1], 20)[0]                    # queries a and b: train a at 20 bits
            dr[b] = bases(rng, 1)[0]
        out.append(_tie_case("hamming_ties-two_queries_%d_%d" % (a, b), (1, a, b), 300, two_queries))

    def identical(rng, kr, dr, kc, dc):
        dr[:] = dr[0]; dc[:] = dr[0]
    out.append(_tie_case("hamming_ties-identical", (2,), 8, identical))
    return out


def chunk_boundary(cap):
    """Boxes whose train list passes through LDS in more than one chunk of 2048.  For the workspace of GEOM_BIG only."""
    assert cap >= 4200, "the chunk-boundary cases need a workspace of at least 4,200 key points per image (has %d)" % cap
    out = []
    for nt in (2047, 2048, 2049, 4097):
        rng = _rng(6, nt)
        partners = sorted({0, 1, nt // 3, nt - 2, nt - 1} | ({2047} if 2047 < nt < 4097 else set()) | ({2048} if 2048 < nt < 4097 else set()))
        x = rng.uniform(4, W - 16, nt); y = rng.uniform(2, 118, nt)
        dr = sc.rand_desc(rng, nt)
        kc = kps(x[partners], y[partners]); dc = sc.flipped(rng, dr[partners], 8)
        note = dict(partners=partners)
        if nt == 4097:
            q = sc.rand_desc(rng, 3)
            for tq, (ta, fa, tb, fb) in zip(q, ((2047, 20, 2048, 20), (100, 20, 2148, 20), (50, 30, 2100, 10))):
                dr[ta] = sc.flipped(rng, tq[None], fa)[0]; dr[tb] = sc.flipped(rng, tq[None], fb)[0]
            kc = np.concatenate([kc, kps(x[[2047, 100, 2100]], y[[2047, 100, 2100]])]); dc = np.concatenate([dc, q])
            note["ties"] = ((2047, 2048), (100, 2148)); note["later_chunk_nearer"] = (50, 2100)
        box = [(0.0, 0.0, float(W), 120.0)]
        st = kps(rng.uniform(4, W - 4, 5), rng.uniform(130, H - 2, 5)); sd = sc.rand_desc(rng, 5)
        ref = frame(np.concatenate([kps(x, y), st]), np.concatenate([dr, sd]), box, [7])
        cur = frame(np.concatenate([kc, st]), np.concatenate([dc, sc.rand_desc(rng, 5)]), box, [7])
        out.append(case("chunk_boundary-nt%d" % nt, ref, cur, cap=cap, **note))
    return out


MATCH_COUNT_GATES = ((2, 2), (3, 3), (15, 3), (16, 3), (50, 10), (51, 10))


def match_count_gates():
    """(nq, ng): ng partnered queries among nq, ng trains; then an ordinary box of 6 pairs, whose matches must overwrite whatever
    a skipped box left in the scratch part of the match list."""
    return [Pair("match_count_gates-nq%d-ng%d" % (nq, ng), 7, nq, ng).box(2, 30, ng, n_cur_extra=nq - ng).box(13, 31, 6).statics(3)
            .case(gate=(nq, ng), skipped=bool(ng < 3 or ng < 0.2 * nq)) for nq, ng in MATCH_COUNT_GATES]


STATIC_COUNT_GATES = ((3, 1), (3, 2), (10, 2), (10, 3), (11, 2), (11, 3), (5, 1), (5, 2))


def static_count_gates():
    """(ng, num0): num0 of ng matches consistent with the model, the others 10 px off.  Alternately H = I and F = [e]x I."""
    out = []
    for k, (ng, num0) in enumerate(STATIC_COUNT_GATES):
        flag = 1 + k % 2
        out.append(Pair("static_count_gates-ng%d-num%d" % (ng, num0), 8, ng, num0).box(6, 2, ng, dyn=range(num0, ng)).statics(2)
                   .case(M=I3 if flag == 1 else F_IDENT, flag=flag, last_idx=[2], last_status=[1], gate=(ng, num0),
                         static=bool(num0 > max(1.0, 0.2 * ng))))
    return out


def status_table():
    """Box 7 is dynamic (6 matches, all 10 px off), box 8 beside it static.  `expect` is box 7's status afterwards."""
    out = []

    def base(name, key, ref_id=None):
        return Pair("status_table-" + name, 9, *key).box(1, 7, 6, dyn=range(6), ref_id=ref_id).box(14, 8, 6).statics(3)
    filler = [50 + j for j in range(63)]
    for name, li, ls, expect in (("absent", [8, 9], [0, 2], 0), ("last_m1", [7], [-1], 0), ("last_0", [9, 7], [1, 0], 2), ("last_1", [7], [1], 0),
                                 ("last_2", [7, 8], [2, 1], 2), ("twice_0_then_1", [7, 7], [0, 1], 2), ("twice_1_then_0", [7, 7], [1, 0], 0),
                                 ("n_last_0", [], [], 0), ("n_last_64", filler + [7], [1] * 63 + [2], 2)):
        out.append(base(name, (len(out),)).case(last_idx=li, last_status=ls, expect=expect, flag=1 + len(out) % 2,
                                                 M=I3 if len(out) % 2 == 0 else F_IDENT))
    out.append(base("absent_from_ref", (20,), ref_id=70).case(last_idx=[7], last_status=[0], expect=-1))
    # the id twice in the reference frame: the first box holds the partners on the spot (box 7 is static and keeps -1), the second holds
    # copies of them 60 px lower: matched against those, box 7 would be dynamic and end at 2
    P = Pair("status_table-twice_in_ref", 9, 21).box(1, 7, 6).box(14, 8, 6).statics(3)
    kr, dr = P.k[0][0].copy(), P.d[0][0].copy()
    kr["y"] += 60.0                                                  # tile 9, below tile 1
    P.add(0, kr, dr); P.add_box(0, P.tile_rect(9), 7)
    out.append(P.case(last_idx=[7], last_status=[0], expect=-1))
    # the box has no key points in the reference / in the current frame: firstSeparate erases it there
    for side in (0, 1):
        P = Pair("status_table-no_keypoints_%s" % ("ref", "cur")[side], 9, 22, side).box(14, 8, 6).statics(3)
        kr, dr, kc, dc = P.matched(1, 6, dyn=range(6))
        P.add(1 - side, (kr, kc)[1 - side], (dr, dc)[1 - side])
        for s in (0, 1):
            P.add_box(s, P.tile_rect(1), 7)
        out.append(P.case(last_idx=[7], last_status=[0], expect=-1 if side == 0 else None))
    return out


def _place(chi, p2, n, lo, hi):
    """Bisection of s in [lo, hi] onto chi(p2 + s * n) == 0 crossing (chi is the f64 statistic minus its threshold)."""
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if chi(p2 + mid * n) > 0:
            hi = mid
        else:
            lo = mid
    return p2 + lo * n


SCAN_HALF = 8            # f32 steps of the current point's x on either side of the threshold
SCANS_PER_BOX, SCAN_BOXES, SCAN_CASES = 16, 4, 4


def threshold_scans(flag):
    """SCAN_CASES cases of SCAN_BOXES boxes of SCANS_PER_BOX scans (256 scans): a reference point, the current point placed by f64
    bisection so that the larger of its two chi-squares equals the threshold, then 17 matches whose current x runs over +-8 f32
    steps around the step nearest the threshold.  General H (not affine), F = [e]x H.  Every box holds 272 matches, all of them
    intended, so every box passes the count gates.  With flag 1 a fifth case holds the exact-arithmetic variant: H = I, v1 == v2,
    u1 - u2 stepped through the f32 grid around sqrt(5.991) (the difference and the inverse are exact, only the square rounds)."""
    th = TH_H if flag == 1 else TH_F
    M32 = (H_GENERAL if flag == 1 else cross(EPI) @ H_GENERAL).astype(F32)
    M = M32.astype(np.float64)
    Hm = H_GENERAL

    def stat(p1, p2):
        c1, c2 = chi2_f64(M, flag, p1[None], p2[None])
        return max(c1[0], c2[0]) - th
    out = []
    for ci in range(SCAN_CASES):
        rng = _rng(10, flag, ci)
        P = Pair("threshold_scans-flag%d-%d" % (flag, ci), 10, flag, ci, 1)
        scans = []
        for bi in range(SCAN_BOXES):
            x0 = 188.0 * bi
            xr, yr, xc, yc = [], [], [], []
            for _ in range(SCANS_PER_BOX):
                p1 = np.array([F32(rng.uniform(x0 + 20, x0 + 150)), F32(rng.uniform(24, 212))], np.float64)
                h = Hm @ np.array([p1[0], p1[1], 1.0]); p2 = h[:2] / h[2]
                if flag == 1:
                    a = rng.uniform(-np.pi / 3, np.pi / 3) + (np.pi if rng.random() < 0.5 else 0.0)      # |cos| >= 0.5: x matters
                    n = np.array([np.cos(a), np.sin(a)])
                else:
                    l = M @ np.array([p1[0], p1[1], 1.0])
                    n = l[:2] / np.hypot(l[0], l[1]) * (1 if rng.random() < 0.5 else -1)
                    p2 = p2 + rng.uniform(-3, 3) * np.array([-n[1], n[0]])                                  # along the line
                q = _place(lambda p: stat(p1, np.array([F32(p[0]), F32(p[1])], np.float64)), p2, n, 0.0, 6.0)
                cx = steps(F32(q[0]), np.arange(-40, 41)); y2 = F32(q[1])
                k0 = int(np.argmin([abs(stat(p1, np.array([np.float64(v), np.float64(y2)]))) for v in cx])) - 40
                xs = steps(F32(q[0]), k0 + np.arange(-SCAN_HALF, SCAN_HALF + 1))
                xr += [p1[0]] * len(xs); yr += [p1[1]] * len(xs); xc += list(xs); yc += [y2] * len(xs)
                scans.append((bi, len(xr) - len(xs), len(xs)))
            n_ = len(xr)
            d = bases(rng, n_)
            P.add(0, kps(np.array(xr, F32), np.array(yr, F32)), d); P.add(1, kps(np.array(xc, F32), np.array(yc, F32)), sc.flipped(rng, d, 6))
            for side in (0, 1):
                P.add_box(side, (x0 + 2.0, 2.0, 184.0, 236.0), bi)
        out.append(P.case(M=M32, flag=flag, scans=scans))
    if flag == 1:
        P = Pair("threshold_scans-flag1-exact", 10, 1, 99)
        rng = P.rng
        xr, xc, y, scans = [], [], [], []
        for s in range(12):
            u1 = F32(40 + 50 * s + (s % 3) * 0.25); v = F32(30 + 7 * s)
            xs = steps(F32(u1 + F32(np.sqrt(TH_H))), np.arange(-SCAN_HALF, SCAN_HALF + 1))
            scans.append((0, len(xr), len(xs)))
            xr += [u1] * len(xs); xc += list(xs); y += [v] * len(xs)
        d = bases(rng, len(xr))
        P.add(0, kps(np.array(xr, F32), np.array(y, F32)), d); P.add(1, kps(np.array(xc, F32), np.array(y, F32)), sc.flipped(rng, d, 6))
        for side in (0, 1):
            P.add_box(side, (0.0, 0.0, float(W), 180.0), 0)
        out.append(P.case(scans=scans))
    return out


def degenerate_models():
    """One box of 10 pairs on the spot, under models that are no models.  `all_dynamic`: what the CPU test pins (the oracle's bytes
    are the expectation either way).  The oracle does NOT call every match dynamic in epipole: [e]x I is a proper F for the nine
    matches off the epipole (p2 == p1 lies on its line); only the match AT the epipole, whose line is a = b = c = 0 and whose
    chi-square is 0 / 0, is dynamic."""
    out = []
    nan, inf = np.nan, np.inf
    models = (
        ("singular_H", 1, [[1, 0, 5], [2, 0, 10], [0, 0, 1]], True),                  # det 0: inverse zeros, 1 / 0, NaN
        ("zero_H", 1, np.zeros((3, 3)), True),
        ("vanishing_line", 1, [[1, 0, 0], [0, 1, 0], [-1 / 128.0, 0, 1]], True),       # the reference point u1 = 128 has w = 0
        ("rank1_F", 2, np.outer([1, 0, -1000.0], [1, 0, -1000.0]), True),              # every line is x = 1000
        ("zero_F", 2, np.zeros((3, 3)), True),
        ("epipole", 2, cross((300.0, 100.0)), False),
        ("nan_H", 1, [[1, 0, 0], [0, nan, 0], [0, 0, 1]], True),
        ("inf_H", 1, [[1, 0, inf], [0, 1, 0], [0, 0, 1]], True),
        ("nan_F", 2, [[0, -1, 100], [1, 0, nan], [-100, 300, 0]], True),
        ("inf_F", 2, [[0, -1, 100], [1, 0, -300], [-100, inf, 0]], True),
    )
    for k, (name, flag, M, all_dyn) in enumerate(models):
        P = Pair("degenerate_models-" + name, 11, k)
        kr, dr, kc, dc = P.matched(11, 10)                              # tile 11: x0 = 282, y0 = 60
        for kk in (kr, kc):
            if name == "vanishing_line":
                kk["x"][0] = 128.0; kk["y"][0] = 70.0
            if name == "epipole":
                kk["x"][0] = 300.0; kk["y"][0] = 100.0
        P.add(0, kr, dr); P.add(1, kc, dc)
        rect = (100.0, 62.0, 272.0, 56.0) if name == "vanishing_line" else P.tile_rect(11)
        for side in (0, 1):
            P.add_box(side, rect, 3)
        out.append(P.statics(2).case(M=np.array(M, np.float64), flag=flag, last_idx=[3], last_status=[2], all_dynamic=all_dyn))
    return out


def readmission():
    """shared: boxes 1 and 2 overlap; 4 key points in box 1 only, 3 in both, 4 in box 2 only, all consistent with H = I: UpdateFrame
    appends the 3 shared ones once, at box 1's position.  ret0: a box of 5 matches with one consistent match: Separate returns 0, so
    UpdateFrame(only_if_static) appends nothing and UpdateFrame(always) appends that one key point."""
    P = Pair("readmission-shared", 12, 0).statics(4)
    x = np.array([110, 120, 130, 140, 160, 170, 180, 210, 220, 230, 240], np.float64); y = 60.0 + 5 * np.arange(11)
    d = bases(P.rng, 11)
    P.add(0, kps(x, y), d); P.add(1, kps(x, y), sc.flipped(P.rng, d, 6))
    for side in (0, 1):
        P.add_box(side, (100.0, 50.0, 100.0, 80.0), 1); P.add_box(side, (150.0, 50.0, 100.0, 80.0), 2)
    shared = P.case(shared=(4, 5, 6))
    ret0 = Pair("readmission-ret0", 12, 1).box(4, 6, 5, dyn=range(1, 5)).statics(4).case(last_idx=[6], last_status=[1])
    return [shared, ret0]


def distort_f64(p):
    """Forward Brown model of DIST_K4 / DIST_D5 on pixel coordinates (the inverse of Frame::UndistortKeyPoints), float64."""
    fx, fy, cx, cy = DIST_K4.astype(np.float64); k1, k2, p1, p2, k3 = DIST_D5.astype(np.float64)
    x = (p[:, 0] - cx) / fx; y = (p[:, 1] - cy) / fy
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x); yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * fx + cx, yd * fy + cy], 1)


DIST_SHIFT = 60.0


def distortion():
    """One box of 24 pairs under a camera with distortion and H = a shift by 60 px in x.  The current key point is the DISTORTED image
    of (undistorted reference point + shift): consistent with H in mvKeysUn, where the classification happens, and several pixels off
    in the raw coordinates."""
    rng = _rng(13)
    xu = rng.uniform(150, 520, 24); yu = rng.uniform(30, 210, 24)
    pr = distort_f64(np.stack([xu, yu], 1)); pc = distort_f64(np.stack([xu + DIST_SHIFT, yu], 1))
    d = bases(rng, 24)
    box = [(100.0, 10.0, 560.0, 220.0)]
    st = kps(np.array([20.0, 40.0, 700.0]), np.array([20.0, 200.0, 120.0])); sd = bases(rng, 3)
    ref = frame(np.concatenate([kps(pr[:, 0], pr[:, 1]), st]), np.concatenate([d, sd]), box, [5])
    cur = frame(np.concatenate([kps(pc[:, 0], pc[:, 1]), st]), np.concatenate([sc.flipped(rng, d, 6), sd]), box, [5])
    Hs = np.array([[1, 0, DIST_SHIFT], [0, 1, 0], [0, 0, 1]], F32)
    return [case("distortion-shift", ref, cur, M=Hs, dist=True, last_idx=[5], last_status=[0])]


def suite():
    """Everything except chunk_boundary (its own workspace) and distortion (its own camera)."""
    return (membership_edges() + empty_box_patterns() + partition_sizes() + match_sizes() + hamming_ties() + match_count_gates()
            + static_count_gates() + status_table() + threshold_scans(1) + threshold_scans(2) + degenerate_models() + readmission())


# ---- the oracle side
def _un(orc, kp):
    out = kp.copy()
    if len(kp):
        u = orc.undistort_points(np.stack([kp["x"], kp["y"]], 1), DIST_K4, DIST_D5)
        out["x"] = u[:, 0]; out["y"] = u[:, 1]
    return out


def oracle_frame(orc, f):
    """orc.first_separate on one frame -> what the device must hold for it after k_box_separate."""
    boxes, ids = (f["boxes"], f["ids"]) if len(f["kp"]) else (np.zeros((0, 4)), np.zeros(0, np.int32))
    nb = len(ids)
    r = orc.first_separate(f["kp"], f["desc"], boxes, ids, np.zeros(nb, np.uint8), np.zeros((nb, 2)))
    kept, _ = np_first_separate(dict(kp=f["kp"], boxes=boxes))
    r["kept_orig"] = np.asarray(kept, np.int32)
    return r


def oracle(orc, c, only_if_static=False):
    """first_separate on both frames, separate, update_frame.  With a distortion the classification reads the undistorted positions
    (mvdynKeysUn), everything else the raw ones."""
    rf, cu = oracle_frame(orc, c["ref"]), oracle_frame(orc, c["cur"])
    side = lambda r: dict(kp=_un(orc, r["kp"]) if c["dist"] else r["kp"], desc=r["desc"], boxStart=r["boxStart"], boxItems=r["boxItems"],
                          box_idx=r["box_idx"])
    nbc = len(cu["box_idx"])
    ret, status, ds, dyn, mt = orc.separate(c["M"], c["flag"], side(cu), side(rf), c["last_idx"], c["last_status"], np.full(nbc, -1, np.int32))
    app = orc.update_frame(cu["kp"], cu["boxStart"], cu["boxItems"], ds, dyn)
    if only_if_static and not ret:
        app = app[:0]
    Ns = cu["Ns"]
    return dict(ref=rf, cur=cu, ret=ret, status=status, dynStart=ds, dyn=dyn, matches=mt, appended=app,
                kp_after=np.concatenate([cu["kp"][:Ns], cu["kp"][app]]), desc_after=np.concatenate([cu["desc"][:Ns], cu["desc"][app]]))


def box_matches(o, b):
    """(matches, dyn) of current box b in an oracle result."""
    s, e = o["dynStart"][b], o["dynStart"][b + 1]
    return o["matches"][s:e], o["dyn"][s:e]


def match_points(o, c, orc=None):
    """Per classified match of the case: (box, p1 reference position, p2 current position, static?), positions as the classification reads them."""
    rf, cu = o["ref"], o["cur"]
    kr, kc = (_un(orc, rf["kp"]), _un(orc, cu["kp"])) if c["dist"] else (rf["kp"], cu["kp"])
    B, P1, P2, S = [], [], [], []
    for b in range(len(cu["box_idx"])):
        mt, dyn = box_matches(o, b)
        if not len(mt):
            continue
        rb = int(np.nonzero(rf["box_idx"] == cu["box_idx"][b])[0][0])
        ic = cu["boxItems"][cu["boxStart"][b] + mt[:, 0]]; ir = rf["boxItems"][rf["boxStart"][rb] + mt[:, 1]]
        B.append(np.full(len(mt), b)); S.append(dyn != -1)
        P1.append(np.stack([kr["x"][ir], kr["y"][ir]], 1)); P2.append(np.stack([kc["x"][ic], kc["y"][ic]], 1))
    if not B:
        return np.zeros(0, int), np.zeros((0, 2), F32), np.zeros((0, 2), F32), np.zeros(0, bool)
    return np.concatenate(B), np.concatenate(P1), np.concatenate(P2), np.concatenate(S)


# ---- the device side (tests marked gpu and tools/fuzz_cull.py)
class Workspace:
    """2 * n_pairs image slots of one geometry: slots 2p / 2p + 1 hold the reference / current frame of pair p."""

    def __init__(self, fe, n_pairs, g=GEOM):
        import torch
        self.fe, self.g, self.n_pairs = fe, g, n_pairs
        self.ex = fe.ORBextractor(*g.extractor_args())
        self.b = fe.Batch(self.ex, g.W, g.H, 2 * n_pairs)
        kp_p, desc_p, cnt_p, self.cap = self.b.results_device()
        n = 2 * n_pairs
        self.kp = fe.as_torch_u8(kp_p, n * self.cap * KP_DTYPE.itemsize).view(n, self.cap * KP_DTYPE.itemsize)
        self.desc = fe.as_torch_u8(desc_p, n * self.cap * 32).view(n, self.cap * 32)
        self.count = fe.as_torch_u8(cnt_p, n * 4).view(torch.int32)
        self.blank = np.full((g.H, g.W), 128, np.uint8)        # the images only make the slots valid

    def close(self):
        self.b.close()


def upload(ws, frames):
    """extract_host once, then frame s of `frames` overwrites slot s's key points, descriptor and count."""
    import torch
    b, n = ws.b, len(frames)
    assert 0 < n <= 2 * ws.n_pairs
    b.extract_host(np.broadcast_to(ws.blank, (n,) + ws.blank.shape))
    b.sync()
    for s, f in enumerate(frames):
        k, d = f["kp"], f["desc"]
        assert len(k) <= ws.cap
        if len(k):
            ws.kp[s, :k.nbytes] = torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda()
            ws.desc[s, :d.size] = torch.from_numpy(d.reshape(-1).copy()).cuda()
    ws.count[:n] = torch.tensor([len(f["kp"]) for f in frames], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()


def download_frame(b, slot):
    g = b.download_boxes(slot)
    g["kp_s"], g["desc_s"], _ = b.download(slot)
    g["kp_d"], g["desc_d"], _, _ = b.download_dynamic(slot)
    return g


def run_cases(ws, cases, only_if_static=False):
    """The device cull on len(cases) cases through ONE first_separate, ONE separate and ONE update_frame launch, everything through the
    public ABI.  -> per case dict(ref, cur (download_frame after separate), ret, dynStart, dyn, matches, count_after, kp_after, desc_after)"""
    b, n = ws.b, len(cases)
    assert 0 < n <= ws.n_pairs
    dist = cases[0]["dist"]
    for c in cases:
        check_domain(c, ws.cap)
        assert c["dist"] == dist, "cases with and without a distortion cannot share a launch"
    upload(ws, [f for c in cases for f in (c["ref"], c["cur"])])
    slots = list(range(2 * n))
    b.set_distortion(DIST_K4, DIST_D5 if dist else np.zeros(5, F32))
    try:
        b.undistort(slots)
        b.first_separate(slots, [f["boxes"] for c in cases for f in (c["ref"], c["cur"])], [f["ids"] for c in cases for f in (c["ref"], c["cur"])])
        b.undistort(slots)            # firstSeparate permuted mvKeys: mvKeysUn / mvdynKeysUn follow (as the tracker does)
        b.separate([2 * p + 1 for p in range(n)], [2 * p for p in range(n)], np.stack([c["M"] for c in cases]), [c["flag"] for c in cases],
                   [c["last_idx"] for c in cases], [c["last_status"] for c in cases])
        out = []
        for p in range(n):
            ret, ds, dyn, mt = b.download_separate(p)
            r = dict(ref=download_frame(b, 2 * p), cur=download_frame(b, 2 * p + 1), ret=ret, dyn=dyn, matches=mt)
            r["dynStart"] = ds[:r["cur"]["nb"] + 1].copy(); r["dynStart_tail"] = ds[r["cur"]["nb"]:].copy()
            if dist:
                r["cur"]["kp_d_un"] = b.download_dynamic_keys_un(2 * p + 1); r["ref"]["kp_d_un"] = b.download_dynamic_keys_un(2 * p)
            out.append(r)
        b.update_frame(only_if_static=only_if_static)
        cnt = b.counts(2 * n)
        for p, r in enumerate(out):
            r["count_after"] = int(cnt[2 * p + 1]); r["ref_count_after"] = int(cnt[2 * p])
            r["kp_after"], r["desc_after"], _ = b.download(2 * p + 1)
    finally:
        b.set_distortion(DIST_K4, np.zeros(5, F32))
    return out


def _diff(bad, name, a, b):
    a = np.asarray(a); b = np.asarray(b)
    if a.dtype.names:
        w = a.dtype.itemsize // 4
        a = np.frombuffer(a.tobytes(), np.uint32).reshape(len(a), w); b = np.frombuffer(b.tobytes(), np.uint32).reshape(len(b), w)
    if a.shape != b.shape:
        bad.append("%s: shape %s vs %s" % (name, a.shape, b.shape))
    elif a.dtype.kind == "f":
        _diff(bad, name, a.view(np.uint64 if a.itemsize == 8 else np.uint32), b.view(np.uint64 if b.itemsize == 8 else np.uint32))
    elif not np.array_equal(a, b):
        i = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
        bad.append("%s differs at %d of %d, first %d: %r vs %r" % (name, len(i), len(a), i[0], a[i[0]], b[i[0]]))


def compare_frame(bad, side, g, r, status, orc=None):
    """One frame's download_frame against its oracle_frame; status = the box statuses expected."""
    Ns = r["Ns"]
    for name, a, b in (("n_static", [g["n_static"]], [Ns]), ("n_all", [g["n_all"]], [Ns + r["Nd"]]), ("nb", [g["nb"]], [len(r["box_idx"])]),
                       ("boxes", g["boxes"], r["boxes"]), ("box_idx", g["box_idx"], r["box_idx"]), ("kept_orig", g["kept_orig"], r["kept_orig"]),
                       ("boxStart", g["boxStart"], r["boxStart"]), ("boxItems", g["boxItems"] + Ns, r["boxItems"]), ("box_status", g["box_status"], status),
                       ("static key points", g["kp_s"], r["kp"][:Ns]), ("static descriptors", g["desc_s"], r["desc"][:Ns]),
                       ("dynamic key points", g["kp_d"], r["kp"][Ns:]), ("dynamic descriptors", g["desc_d"], r["desc"][Ns:])):
        _diff(bad, "%s %s" % (side, name), a, b)
    if "kp_d_un" in g and orc is not None:
        _diff(bad, "%s mvdynKeysUn" % side, g["kp_d_un"], _un(orc, r["kp"][Ns:]))
    return bad


def compare(got, o, orc=None):
    """What of a device result differs from the oracle's: a list of strings (field name and first index)."""
    bad = []
    compare_frame(bad, "ref", got["ref"], o["ref"], np.full(len(o["ref"]["box_idx"]), -1), orc)
    compare_frame(bad, "cur", got["cur"], o["cur"], o["status"], orc)
    _diff(bad, "ret", [got["ret"]], [o["ret"]])
    _diff(bad, "dynStart", got["dynStart"], o["dynStart"])
    _diff(bad, "dynStart beyond nb", got["dynStart_tail"], np.full(len(got["dynStart_tail"]), o["dynStart"][-1]))
    _diff(bad, "dynStatus", got["dyn"], o["dyn"])
    _diff(bad, "matches", got["matches"], o["matches"])
    _diff(bad, "count after UpdateFrame", [got["count_after"]], [len(o["kp_after"])])
    _diff(bad, "reference count after UpdateFrame", [got["ref_count_after"]], [o["ref"]["Ns"]])
    _diff(bad, "key points after UpdateFrame", got["kp_after"], o["kp_after"])
    _diff(bad, "descriptors after UpdateFrame", got["desc_after"], o["desc_after"])
    return bad


def result_bytes(r):
    """Everything run_cases returns for a case as one bytes object (slot- and launch-independent)."""
    parts = []
    for side in ("ref", "cur"):
        g = r[side]
        parts += [np.array([g["nb"], g["n_all"], g["n_static"]]), g["boxes"], g["box_idx"], g["box_status"], g["kept_orig"], g["boxStart"], g["boxItems"],
                  g["kp_s"], g["desc_s"], g["kp_d"], g["desc_d"]]
    parts += [np.array([r["ret"], r["count_after"], r["ref_count_after"]]), r["dynStart"], r["dyn"], r["matches"], r["kp_after"], r["desc_after"]]
    return b"|".join(np.ascontiguousarray(p).tobytes() for p in parts)
