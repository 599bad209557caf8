"""Shared by test_bow_cases.py and test_gpu_bow_cases.py: crafted vocabulary trees and descriptors for the three kernels of k_bow.h
(k_bow_transform, k_bow_finalize = Frame::ComputeBoW; k_search_by_bow = ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...)), numpy
restatements of the three that share no code with the oracle, and the device drivers.

A vocabulary is a hand-built node list in the dict format of synth.vocabulary (node id = line + 1, parents before children, children in
file order).  Every group returns the tree, the descriptors that exercise it and, per descriptor, a name saying what it was built for
plus a claim that test_bow_cases.py recomputes from the bits.  The keyframe-frame pairs live on triangulate_cases.vocabulary: features
are identities and candidates of triangulate_cases.Descriptors, so node membership and every distance that matters are chosen.

Each restatement takes mutant=<name>: one deliberate error.  test_bow_cases.py shows that the cases tell every mutant from the oracle.
Seeds depend on the kind of case and its parameters only."""
import math

import numpy as np

import triangulate_cases as tc
from triangulate_cases import F32, KeyFrameBuilder, T1_DEFAULT

TH_LOW, HISTO = 50, 30
REGF = 128                # SD_BOW_REGF: frame features of a node that the register path of k_search_by_bow holds
SIZES = (0, 1, 15, 16, 17, 255, 256, 257, 512, 513, 1024, 1025)
GEOM_BIG = dict(tc.GEOM, nfeatures=1100)         # a workspace whose capacity is at least 1025 (its images are never read)
TRANSFORM_MUTANTS = ("last_min", "round_local_tie", "nid_zero_when_unset")
VECTOR_MUTANTS = ("c_times_w", "pairwise_norm", "reverse_norm", "keep_zero_weight", "sort_by_word_only")
KF_FRAME_MUTANTS = ("th_low_exclusive", "ratio_le", "ignore_taken", "second_best_includes_taken", "mask_by_kf_slot", "hist_first_two",
                    "round_half_even")


def sort_size(n):
    """k_bow_finalize's sort size for an image of n key points, and the items each of its 256 threads owns."""
    s = 256
    while s < n:
        s <<= 1
    return s, s // 256


# ---------------------------------------------------------------- hand-built trees
class Tree:
    def __init__(self, k, L):
        self.k, self.L = k, L
        self.parent, self.leaf, self.desc, self.weight = [], [], [], []

    def add(self, parent, desc, weight=None):
        """weight None: an interior node.  -> the node id."""
        self.parent.append(parent); self.leaf.append(0 if weight is None else 1)
        self.desc.append(np.asarray(desc, np.uint8).copy()); self.weight.append(0.0 if weight is None else float(weight))
        return len(self.parent)

    def build(self, scoring=0, weighting=0):
        return dict(k=self.k, L=self.L, scoring=scoring, weighting=weighting, parent=np.array(self.parent, np.int32),
                    is_leaf=np.array(self.leaf, np.uint8), desc=np.array(self.desc, np.uint8).reshape(-1, 32), weight=np.array(self.weight, np.float64))


def children_of(voc):
    """[node id] -> child ids in file order; descriptors and weights indexed by node id (root = 0)."""
    n = len(voc["parent"])
    ch = [[] for _ in range(n + 1)]
    for line in range(n):
        ch[int(voc["parent"][line])].append(line + 1)
    desc = np.concatenate([np.zeros((1, 32), np.uint8), np.asarray(voc["desc"], np.uint8)])
    weight = np.concatenate([[0.0], np.asarray(voc["weight"], np.float64)])
    word = np.full(n + 1, -1, np.int64)
    word[1:][np.asarray(voc["is_leaf"]) > 0] = np.arange(int((np.asarray(voc["is_leaf"]) > 0).sum()))
    return ch, desc, weight, word


def with_scoring(voc, scoring, weighting):
    v = dict(voc); v["scoring"], v["weighting"] = scoring, weighting
    return v


def with_zero_weights(voc):
    v = dict(voc); v["weight"] = np.zeros_like(voc["weight"])
    return v


def dists(d, D):
    return np.unpackbits(np.bitwise_xor(np.asarray(D, np.uint8).reshape(-1, 32), np.asarray(d, np.uint8)[None, :]), axis=1).sum(1).astype(np.int64)


def _block(j, w):
    return list(range(w * j, w * j + w))


def _tie_block(j):
    """Children 3 and 17 share a block (the same descriptor); the other 18 children have blocks of their own."""
    return 3 if j == 17 else (j if j < 17 else j - 1)


def ties():
    """k = 20, L = 2.  Level 1: child j = B with its own 12-bit block flipped, so B is 12 from every child, a half-and-half mix of two
    blocks is 12 from those two and 24 from the rest, and the complement of a child is 256 from it and 232 from the rest.  Child 7
    repeats the plan with 4-bit blocks inside bits 0 .. 75 (a probe with up to 8 of them flipped stays nearer to child 7 than to any
    other level-1 child); child 9 holds 19 copies of the complement of its own descriptor and one child 10 bits from that.
    -> dict(voc, desc, names, claims): claims[i] = (parent node, level, tied child positions, their distance)."""
    rng = np.random.default_rng(4101)
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    T = Tree(20, 2)
    c1 = [tc._flip(B, _block(_tie_block(j), 12)) for j in range(20)]
    ids1 = [T.add(0, c1[j], None if j in (7, 9) else rng.uniform(0.5, 9.0)) for j in range(20)]
    B7 = c1[7]
    c2 = [tc._flip(B7, _block(_tie_block(j), 4)) for j in range(20)]
    for j in range(20):
        T.add(ids1[7], c2[j], rng.uniform(0.5, 9.0))
    X = np.bitwise_not(c1[9])
    for j in range(20):
        T.add(ids1[9], tc._flip(X, range(240, 250)) if j == 12 else X, rng.uniform(0.5, 9.0))
    half = lambda a, b, w: _block(_tie_block(a), w)[:w // 2] + _block(_tie_block(b), w)[w // 2:]
    probes = [
        ("l1_duplicate_3_17", c1[3], (0, 1, [3, 17], 0)),
        ("l1_duplicate_3_17_at_5", tc._flip(c1[3], range(230, 235)), (0, 1, [3, 17], 5)),
        ("l1_tie_5_6", tc._flip(B, half(5, 6, 12)), (0, 1, [5, 6], 12)),
        ("l1_tie_2_18_one_lane", tc._flip(B, half(2, 18, 12)), (0, 1, [2, 18], 12)),
        ("l1_tie_15_16_round_edge", tc._flip(B, half(15, 16, 12)), (0, 1, [15, 16], 12)),
        ("l1_all_equal", B, (0, 1, list(range(20)), 12)),
        ("l1_all_equal_at_22", tc._flip(B, range(230, 240)), (0, 1, list(range(20)), 22)),
        ("l1_second_round_alone", c1[18], (0, 1, [18], 0)),
        ("l1_complement_of_4", np.bitwise_not(c1[4]), (0, 1, [j for j in range(20) if j != 4], 232)),
        ("l1_complement_of_0", np.bitwise_not(c1[0]), (0, 1, list(range(1, 20)), 232)),
        ("l2_duplicate_3_17", c2[3], (ids1[7], 2, [3, 17], 0)),
        ("l2_tie_5_6", tc._flip(B7, half(5, 6, 4)), (ids1[7], 2, [5, 6], 4)),
        ("l2_tie_2_18_one_lane", tc._flip(B7, half(2, 18, 4)), (ids1[7], 2, [2, 18], 4)),
        ("l2_all_equal", B7, (ids1[7], 2, list(range(20)), 4)),
        ("l2_second_round_alone", c2[19], (ids1[7], 2, [19], 0)),
        ("l2_256_from_all_but_one", c1[9], (ids1[9], 2, [12], 246)),
    ]
    return dict(voc=T.build(), desc=np.array([p[1] for p in probes], np.uint8), names=[p[0] for p in probes], claims=[p[2] for p in probes])


def depths():
    """k = 3, L = 5, leaves at levels 1, 2, 3 and 5 and an interior node with one child.  Features come in fours that descend to depths
    1, 2, 3, 5 in turn: neighbouring 16-lane groups of one wave leave the descent loop after different numbers of rounds.
    -> dict(voc, desc, names, claims): claims[i] = (leaf node id, its level)."""
    rng = np.random.default_rng(4202)
    T = Tree(3, 5)
    near = lambda d, n=16: tc._flip(d, rng.choice(256, n, replace=False))
    w = lambda: rng.uniform(0.5, 9.0)
    root = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3)]
    leaf, dsc = {}, {}

    def node(name, parent, d, lvl, interior=False):
        dsc[name] = d
        i = T.add(parent, d, None if interior else w())
        if not interior:
            leaf[name] = (i, lvl)
        return i

    node("A", 0, root[0], 1); b = node("B", 0, root[1], 1, True); c = node("C", 0, root[2], 1, True)
    node("B0", b, near(root[1]), 2); b1 = node("B1", b, near(root[1]), 2, True); node("B2", b, near(root[1]), 2)
    node("B10", b1, near(dsc["B1"]), 3); b11 = node("B11", b1, near(dsc["B1"]), 3, True); node("B12", b1, near(dsc["B1"]), 3)
    b110 = node("B110", b11, near(dsc["B11"]), 4, True)                       # the only child of B11
    for j in range(3):
        node("B110%d" % j, b110, near(dsc["B110"]), 5)
    node("C0", c, near(root[2]), 2); node("C1", c, near(root[2]), 2); c2 = node("C2", c, near(root[2]), 2, True)
    node("C20", c2, near(dsc["C2"]), 3); node("C21", c2, near(dsc["C2"]), 3)   # two children where k = 3
    fours = [("A", "B0", "B10", "B1101"), ("A", "B2", "B12", "B1100"), ("A", "C1", "C21", "B1102"), ("A", "C0", "C20", "B1101")]
    desc, names, claims = [], [], []
    for q in range(16):                                                       # 64 features: four waves of k_bow_transform
        for name in fours[q % 4]:
            desc.append(near(dsc[name], 3)); names.append("depth%d_%s" % (leaf[name][1], name)); claims.append(leaf[name])
    return dict(voc=T.build(), desc=np.array(desc, np.uint8), names=names, claims=claims, single_child=b11)


WEIGHT_SEED = 10          # the first seed at which c * w, the pairwise and the reversed norm all differ from the reference's sums, under L1 and L2
ZERO_WORDS = (7, 23, 58, 91)
HITS = {3: 1, 14: 2, 25: 3, 36: 5, 47: 7, 69: 70, 7: 2, 58: 1}             # word -> features that land on it (7 and 58 weigh nothing)


def weights_tree(seed=WEIGHT_SEED):
    """k = 10, L = 2, 100 words 60 bits from their siblings; weights with full mantissas over 12 decades, four of them 0."""
    rng = np.random.default_rng(4300 + seed)
    T = Tree(10, 2)
    top = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(10)]
    ids = [T.add(0, d) for d in top]
    for j in range(10):
        for q in range(10):
            wd = 10 * j + q
            T.add(ids[j], tc._flip(top[j], rng.choice(256, 30, replace=False)), 0.0 if wd in ZERO_WORDS else rng.uniform(1.0, 2.0) * 10.0 ** rng.uniform(-6.0, 6.0))
    return T.build()


def word_desc(voc, word):
    return voc["desc"][np.nonzero(voc["is_leaf"])[0][word]]


def frame_on_words(voc, words, rng):
    """One feature per entry of `words`, 4 bits from the word's descriptor."""
    d = [tc._flip(word_desc(voc, int(wd)), rng.choice(256, 4, replace=False)) for wd in words]
    return np.array(d, np.uint8).reshape(len(words), 32)


def weights(seed=WEIGHT_SEED):
    """The HITS on weights_tree plus 30 words hit once, in interleaved feature order.  -> dict(voc, desc, names, claims = the word)."""
    voc = weights_tree(seed)
    rng = np.random.default_rng(4400 + seed)
    words = [wd for wd, c in HITS.items() for _ in range(c)]
    others = [wd for wd in range(100) if wd not in HITS and wd not in ZERO_WORDS]
    words += [int(x) for x in rng.choice(others, 30, replace=False)]
    words = [words[i] for i in rng.permutation(len(words))]
    names = ["word%d_x%d%s" % (wd, HITS.get(wd, 1), "_zero" if wd in ZERO_WORDS else "") for wd in words]
    return dict(voc=voc, desc=frame_on_words(voc, words, rng), names=names, claims=words)


SIZE_SEEDS = {}           # N -> seed, where the default (N) does not give the straddles sizes() promises


def sized_frame(voc, n, seed=None):
    """n features on random words (a third of them on ten favourites, so that words repeat)."""
    rng = np.random.default_rng(4500 + (SIZE_SEEDS.get(n, n) if seed is None else seed))
    fav = rng.choice(100, 10, replace=False)
    words = np.where(rng.random(n) < 0.33, fav[rng.integers(0, 10, n)], rng.integers(0, 100, n))
    return words.astype(np.int64), frame_on_words(voc, words, rng)


def sizes(seed=WEIGHT_SEED):
    """weights_tree with N key points for every N of SIZES, and: 64 and 65 distinct words, every feature on one word, IDF-style repeats.
    -> dict(voc, frames {name: desc}, words {name: word per feature})"""
    voc = weights_tree(seed)
    frames, words = {}, {}
    for n in SIZES:
        words["n%d" % n], frames["n%d" % n] = sized_frame(voc, n)
    rng = np.random.default_rng(4600)
    good = [wd for wd in range(100) if wd not in ZERO_WORDS]
    for nb in (64, 65):
        ws = list(rng.choice(good, nb, replace=False))
        ws = ws + ws[:9] + [ZERO_WORDS[0]]                                    # nine of them twice, one weightless feature
        ws = [ws[i] for i in rng.permutation(len(ws))]
        words["nb%d" % nb] = np.array(ws, np.int64); frames["nb%d" % nb] = frame_on_words(voc, ws, rng)
    words["one_word"] = np.full(40, 69, np.int64); frames["one_word"] = frame_on_words(voc, words["one_word"], rng)
    return dict(voc=voc, frames=frames, words=words)


def straddles(word, weight, nid):
    """Of one image: does a FeatureVector run, and does a repeated word of the BowVector, lie on both sides of a boundary between two
    threads' chunks of k_bow_finalize (sorted positions that are multiples of sortN / 256)?  -> (run, word, per)"""
    n = len(word)
    per = sort_size(n)[1]
    keep = np.nonzero(np.asarray(weight) > 0)[0]
    out = []
    for key in (np.asarray(nid)[keep], np.asarray(word)[keep]):
        s = np.sort(key, kind="stable")
        pos = np.arange(per, len(s), per)
        out.append(bool(per > 1 and len(pos) and np.any(s[pos] == s[pos - 1])))
    return out[0], out[1], per


# ---------------------------------------------------------------- numpy restatements: the transform and the two vectors
def numpy_transform(voc, desc, levelsup, mutant=None):
    """TemplatedVocabulary::transform(feature, word, weight, nid, levelsup) per descriptor: at every node the first child at the
    smallest distance, in file order; nid = the node passed at level L - levelsup, 0 when that level is the root or above, the leaf
    when the descent ended before it (the project's rule where the reference leaves it unwritten)."""
    ch, nd, nw, nword = children_of(voc)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    N = len(desc)
    word = np.zeros(N, np.uint32); weight = np.zeros(N, np.float64); nid = np.zeros(N, np.uint32)
    nid_level = int(voc["L"]) - levelsup
    for i in range(N):
        node, level, got = 0, 0, None
        while ch[node]:
            c = ch[node]
            d = dists(desc[i], nd[c])
            if mutant == "last_min":
                j = len(d) - 1 - int(np.argmin(d[::-1]))
            elif mutant == "round_local_tie":
                j, best = 0, None
                for r in range(0, len(d), 16):
                    jr = r + int(np.argmin(d[r:r + 16]))
                    if best is None or d[jr] <= best:
                        j, best = jr, d[jr]
            else:
                j = int(np.argmin(d))
            node = c[j]; level += 1
            if level == nid_level:
                got = node
        if nid_level <= 0:
            got = 0
        elif got is None:
            got = 0 if mutant == "nid_zero_when_unset" else node
        word[i], weight[i], nid[i] = nword[node], nw[node], got
    return word, weight, nid


def _pairwise(v):
    if len(v) <= 2:
        return sum(v, 0.0)
    h = len(v) // 2
    return _pairwise(v[:h]) + _pairwise(v[h:])


def numpy_bow_vectors(voc, word, weight, nid, mutant=None):
    """transform(features, BowVector, FeatureVector, levelsup) from the per-feature results, in Python floats (IEEE doubles, one
    rounding per operation): a word's value is its weight added once per feature in feature order (TF-IDF, TF) or its weight (IDF,
    BINARY); without a norm (DOT_PRODUCT) TF values are divided by the number of words; otherwise by the L1 norm (L2 for L2_NORM),
    summed in ascending word order.  The FeatureVector lists the weighted features by (node, feature index)."""
    scoring, weighting = int(voc["scoring"]), int(voc["weighting"])
    keep = [i for i in range(len(word)) if float(weight[i]) > 0 or mutant == "keep_zero_weight"]
    if mutant == "sort_by_word_only":
        order = sorted(keep, key=lambda i: (int(nid[i]), -i))
    else:
        order = sorted(keep, key=lambda i: (int(nid[i]), i))
    bow, cnt = {}, {}
    for i in keep:
        wd, w = int(word[i]), float(weight[i])
        cnt[wd] = cnt.get(wd, 0) + 1
        if wd not in bow:
            bow[wd] = w
        elif weighting in (0, 1):
            bow[wd] = bow[wd] + w
    if mutant == "c_times_w" and weighting in (0, 1):
        first = {}
        for i in keep:
            first.setdefault(int(word[i]), float(weight[i]))
        bow = {wd: cnt[wd] * first[wd] for wd in bow}
    ids = sorted(bow)
    vals = [bow[wd] for wd in ids]
    if scoring == 5:
        if weighting in (0, 1) and ids:
            vals = [v / float(len(ids)) for v in vals]
    else:
        terms = [v * v for v in vals] if scoring == 1 else [abs(v) for v in vals]
        if mutant == "pairwise_norm":
            norm = _pairwise(terms)
        else:
            norm = 0.0
            for t in (terms[::-1] if mutant == "reverse_norm" else terms):
                norm = norm + t
        if scoring == 1:
            norm = math.sqrt(norm)
        if norm > 0.0:
            vals = [v / norm for v in vals]
    return dict(word=np.array(ids, np.uint32), value=np.array(vals, np.float64), fv_node=np.array([nid[i] for i in order], np.uint32),
                fv_feature=np.array(order, np.uint32))


def oracle_bow(O, desc, levelsup):
    """The oracle's transform and vectors of one image in the layout of Batch.download_bow."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    if not len(desc):
        z = np.zeros(0, np.uint32)
        return dict(word=z, value=np.zeros(0), fv_node=z, fv_feature=z, f_word=z, f_weight=np.zeros(0), f_node=z)
    word, w, nid = O.transform(desc, levelsup)
    out = O.compute_bow(desc, levelsup)
    out.update(f_word=word, f_weight=w, f_node=nid)
    return out


def numpy_bow(voc, desc, levelsup, mutant=None):
    tm = mutant if mutant in TRANSFORM_MUTANTS else None
    word, w, nid = numpy_transform(voc, desc, levelsup, tm)
    out = numpy_bow_vectors(voc, word, w, nid, None if tm else mutant)
    out.update(f_word=word, f_weight=w, f_node=nid)
    return out


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if len(a) != len(b):
        return min(len(a), len(b))
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    bad = np.nonzero(a != b)[0]
    return int(bad[0]) if len(bad) else None


def _show(a, i):
    """Entry i of a result array; an f64 value as its hex digits (two values that differ in the last bit print alike in decimal)."""
    if i >= len(a):
        return "none"
    return float(a[i]).hex() if np.asarray(a).dtype == np.float64 else str(int(a[i]))


def same_transform(got, want, names, what=""):
    """Per feature word, weight (bits) and node; names the first feature that differs and what it was built for."""
    for f in ("f_word", "f_weight", "f_node"):
        i = _first_diff(got[f], want[f])
        assert i is None, "%s: %s differs at feature %d (%s): %s vs %s (%d / %d features)" % (
            what, f, i, names[i] if i < len(names) else "?", _show(got[f], i), _show(want[f], i), len(got[f]), len(want[f]))


def same_vectors(got, want, what=""):
    """BowVector ids and values (bits), FeatureVector nodes and features."""
    for f in ("word", "value", "fv_node", "fv_feature"):
        i = _first_diff(got[f], want[f])
        assert i is None, "%s: %s differs at entry %d: %s vs %s (%d / %d entries)" % (what, f, i, _show(got[f], i), _show(want[f], i), len(got[f]), len(want[f]))


def differs(a, b, fields):
    return any(_first_diff(a[f], b[f]) is not None for f in fields)


# ---------------------------------------------------------------- keyframe-frame pairs
class FramePair:
    """A keyframe and a frame over the identities of one vocabulary (the PairBuilder of loop_cases.py with a mask on the keyframe only)."""

    def __init__(self, D, seed):
        self.D, self.rng = D, np.random.default_rng(9000 + seed)
        self.K, self.F = KeyFrameBuilder(T1_DEFAULT), KeyFrameBuilder(T1_DEFAULT)
        self.valid, self.k = [], {}
        self.want, self.expect = {}, {}

    def ident(self, slot):
        self.k[slot] = self.k.get(slot, 0) + 1
        return self.D.identity(slot, self.k[slot] - 1)

    def _add(self, B, desc, angle):
        return B.add(float(self.rng.uniform(20, 1200)), float(self.rng.uniform(10, 360)), desc, 0, angle)

    def kf(self, desc, angle=0.0, valid=True):
        self.valid.append(1 if valid else 0)
        return self._add(self.K, desc, angle)

    def fr(self, desc, angle=0.0):
        return self._add(self.F, desc, angle)

    def near(self, ident, d):
        return self.D.candidate(ident, d)

    def build(self, name, O, nnratio=0.75, check_orientation=False, levelsup=tc.LEVELSUP, zero=(), no_mask=False, **kw):
        """zero: the sides ("kf", "frame") whose vocabulary weighs nothing (an empty FeatureVector over N > 0 key points)."""
        k, f = self.K.build(), self.F.build()
        tc.attach_bow([k, f], O, levelsup)
        e = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        if "kf" in zero:
            k["fv"] = e
        if "frame" in zero:
            f["fv"] = e
        c = dict(name=name, kf=k, frame=f, nnratio=nnratio, check_orientation=check_orientation, levelsup=levelsup, zero=tuple(zero),
                 valid=None if no_mask else np.array(self.valid, np.uint8), want=self.want, expect=self.expect, notes={})
        c.update(kw)
        return c


def _level2_prototypes(voc, per_parent=2):
    first = np.nonzero(voc["parent"] == 0)[0] + 1
    out = []
    for p in first:
        out += [voc["desc"][line] for line in np.nonzero(voc["parent"] == p)[0][:per_parent]]
    return out


def _edges(D, O, voc, nnratio):
    """Node slots: 0 keyframe only (below every frame node), 1 distance 50, 2 distance 51, 3 / 4 the ratio edge and the masked feature,
    5 a single free candidate, 6 frame only, 7 / 8 plain, 9 keyframe only (above every frame node)."""
    P = FramePair(D, 1)
    ex, want, notes = P.expect, P.want, {}
    P.kf(P.ident(0)); P.kf(P.ident(9)); P.fr(P.ident(6))
    i = P.ident(1); a = P.kf(i); b = P.fr(P.near(i, 50)); want[(a, b)] = 50; ex[b] = a; notes["d50"] = (a, b)
    i = P.ident(2); a = P.kf(i); b = P.fr(P.near(i, 51)); want[(a, b)] = 51; ex[b] = -1; notes["d51"] = (a, b)
    r = float(F32(nnratio))
    ratio = []
    for q, d2 in enumerate((20, 40, 44, 48, 50)):
        for d1 in (int(math.floor(r * d2)) - 1, int(math.floor(r * d2)), int(math.floor(r * d2)) + 1):
            i = P.ident(3 + q % 2); a = P.kf(i); b = P.fr(P.near(i, d1)); c = P.fr(P.near(i, d2))
            want[(a, b)] = d1; want[(a, c)] = d2
            ratio.append((a, b, d1, d2))
    notes["ratio"] = ratio
    i = P.ident(3); a = P.kf(i, valid=False); b = P.fr(P.near(i, 5)); want[(a, b)] = 5; ex[b] = -1; notes["masked"] = (a, b)
    i = P.ident(5); a = P.kf(i); b = P.fr(P.near(i, 20)); want[(a, b)] = 20; ex[b] = a; notes["single"] = (a, b)
    for s in (7, 8):
        i = P.ident(s); a = P.kf(i); b = P.fr(P.near(i, 12)); want[(a, b)] = 12; ex[b] = a
    return P.build("edges_%g" % nnratio, O, nnratio=nnratio, notes=notes)


def _many_nodes(O, voc, no_mask):
    """20 shared nodes at levelsup 1 (more than the 16 waves of a workgroup): the level-2 descriptors themselves and 3-bit neighbours."""
    P = FramePair(None, 2)
    for d in _level2_prototypes(voc):
        a = P.kf(d); b = P.fr(tc._flip(d, P.rng.choice(256, 3, replace=False))); P.expect[b] = a
    return P.build("many_nodes" + ("_no_mask" if no_mask else ""), O, nnratio=0.75, levelsup=1, no_mask=no_mask, want=None)


def _contention(D, O):
    P = FramePair(D, 3)
    ex, want = P.expect, P.want
    # slot 0: the later keyframe feature takes its next best; slot 1: it fails the ratio (40 against 44)
    i = P.ident(0); f = P.fr(i); a = P.kf(P.near(i, 10)); bd = P.near(i, 20); b = P.kf(bd)
    g = P.fr(tc._flip(bd, P.rng.choice(256, 40, replace=False))); ex[f] = a; ex[g] = b
    i = P.ident(1); f = P.fr(i); a = P.kf(P.near(i, 10)); bd = P.near(i, 20); b = P.kf(bd)
    g = P.fr(tc._flip(bd, P.rng.choice(256, 40, replace=False))); h = P.fr(tc._flip(bd, P.rng.choice(256, 44, replace=False)))
    ex[f] = a; ex[g] = -1; ex[h] = -1
    # slot 2: the two at positions 63 and 64 of a 70-feature keyframe node (the taken flag crosses a 64-block)
    for q in range(63):
        P.kf(P.ident(2))
    i = P.ident(2); f = P.fr(i); a = P.kf(P.near(i, 10)); bd = P.near(i, 20); b = P.kf(bd)
    g = P.fr(tc._flip(bd, P.rng.choice(256, 40, replace=False))); ex[f] = a; ex[g] = b
    for q in range(5):
        P.kf(P.ident(2))
    pos63 = (a, b)
    # slot 3: the contended frame feature at position 64 or beyond of its node (the lane's second register slot)
    for q in range(66):
        P.fr(P.ident(3))
    i = P.ident(3); f = P.fr(i); a = P.kf(P.near(i, 10)); bd = P.near(i, 20); b = P.kf(bd)
    g = P.fr(tc._flip(bd, P.rng.choice(256, 40, replace=False))); ex[f] = a; ex[g] = b
    return P.build("contention", O, nnratio=0.75, want=None, notes=dict(pos63=pos63, second_slot=(f, g)))


def _node_size(D, O, n):
    """A frame node of n features, the close candidates last (they lie on either side of positions 64 / 128 of the node's list), 12
    keyframe features that each have one of them and two that find theirs taken; at 129 the pair also holds small nodes, which take the
    register path in the same workgroup."""
    P = FramePair(D, 10 + n)
    ids = [P.ident(0) for _ in range(12)]
    for q in range(n):
        P.fr(P.near(ids[q % 12], int(P.rng.integers(38, 49)) if q < n - 12 else int(P.rng.integers(5, 13))))
    for q in range(12):
        P.kf(P.near(ids[q], int(P.rng.integers(0, 8))))
    for q in (0, 5):                                         # two more that prefer a candidate already taken: the taken flags of this path
        P.kf(P.near(ids[q], 9))
    if n == 129:
        for s in (1, 4, 7):
            for q in range(3):
                i = P.ident(s); a = P.kf(i); b = P.fr(P.near(i, 5 + q)); P.expect[b] = a
    return P.build("nodeF_%d" % n, O, nnratio=0.9, want=None)


def _rotation_plan(D, O, name, plan, check_orientation, culled):
    P = FramePair(D, 40)
    for q, (aK, aF) in enumerate(plan):
        i = P.ident(q % 10); a = P.kf(i, angle=aK); b = P.fr(P.near(i, 6), angle=aF)
        P.expect[b] = -1 if (check_orientation and q in culled) else a
    return P.build(name, O, nnratio=0.9, check_orientation=check_orientation, want=None)


ROTATION_PLAN = ([(0.0, 0.0)] * 11 + [(899.0, 0.0)] + [(130.0, 10.0)] * 12 + [(357.0, 2.5)] * 6 + [(2.5, 8.0)] * 6 + [(10.0, 130.0)])


def _tenth(n):
    """n matches at 0 degrees and one at 90: max2 < 0.1f * max1 on either side (10: 1 < 1.0f is false; 11: 1 < 1.1f)."""
    return [(0.0, 0.0)] * n + [(100.0, 10.0)]


def bin_edge(orc, O, D):
    """The largest keyframe angle (frame angle 0) that still falls in bin 0, found by bisection with the ORACLE on a pair of 12 matches:
    11 at 30 degrees (bin 1) and the probe, which is removed while it is alone in bin 0."""
    def in_bin0(x):
        c = _rotation_plan(D, O, "probe", [(30.0, 0.0)] * 11 + [(float(x), 0.0)], True, ())
        m, _ = oracle_kf_frame(orc, c)
        return m[11] < 0

    lo, hi = F32(10.0), F32(20.0)
    assert in_bin0(lo) and not in_bin0(hi)
    while hi.view(np.int32) - lo.view(np.int32) > 1:
        mid = np.int32((int(lo.view(np.int32)) + int(hi.view(np.int32))) // 2).view(F32)
        if in_bin0(mid):
            lo = mid
        else:
            hi = mid
    return lo


def scan_case(orc, O, D, steps=16, base=170):
    """`steps` consecutive f32 keyframe angles centred on the edge between bins 0 and 1, over `base` matches in bin 1: a probe in bin 0
    is removed (steps < base / 10), one in bin 1 stays, so the match set shows every probe's bin."""
    lo = bin_edge(orc, O, D)
    first = int(lo.view(np.int32)) - steps // 2 + 1
    probes = (first + np.arange(steps)).astype(np.int32).view(F32)
    c = _rotation_plan(D, O, "scan", [(30.0, 0.0)] * base + [(float(x), 0.0) for x in probes], True, ())
    c["expect"] = {}
    c["notes"] = dict(first_probe=base, probes=probes, edge=lo)
    return c


def _empty(D, O, kind):
    P = FramePair(D, 50)
    i = P.ident(0)
    if kind != "n0_kf":
        P.kf(i)
    if kind != "n0_frame":
        b = P.fr(P.near(i, 5)); P.expect[b] = -1
    zero = {"zero_kf": ("kf",), "zero_frame": ("frame",)}.get(kind, ())
    return P.build("empty_" + kind, O, want=None, zero=zero)


def _masks(D, O):
    """One keyframe against two frames in one call; the mask rows differ, so every feature matches in exactly one of the pairs."""
    P = FramePair(D, 60)
    for q in range(8):
        i = P.ident(q); a = P.kf(i); P.fr(P.near(i, 6 + q))
    c0 = P.build("masks_a", O, want=None)
    c1 = dict(c0); c1["name"] = "masks_b"
    c0["valid"] = np.array([1, 0] * 4, np.uint8); c1["valid"] = np.array([0, 1] * 4, np.uint8)
    c0["expect"] = {q: (q if q % 2 == 0 else -1) for q in range(8)}; c1["expect"] = {q: (q if q % 2 == 1 else -1) for q in range(8)}
    return [c0, c1]


def kf_frame_cases(synth, orc, O=None):
    """-> (voc, {group: [case]}).  A case: dict(name, kf, frame, valid, nnratio, check_orientation, levelsup, zero, want {(iK, iF): d} or
    None, expect {frame feature: keyframe feature or -1}, notes)."""
    voc = tc.vocabulary(synth, 5)
    O = O or orc.Vocabulary.from_nodes(voc)
    D = tc.Descriptors(voc, 1900)
    g = {}
    g["edges"] = [_edges(D, O, voc, 0.7), _edges(D, O, voc, 0.75), _many_nodes(O, voc, False), _many_nodes(O, voc, True)]
    P = FramePair(D, 4)
    i = P.ident(2); a = P.kf(i); b1 = P.fr(P.near(i, 15)); b2 = P.fr(P.near(i, 15)); P.want.update({(a, b1): 15, (a, b2): 15})
    first = P.build("tie_1.5", O, nnratio=1.5); first["expect"] = {b1: a, b2: -1}
    none = dict(first); none.update(name="tie_0.9", nnratio=0.9, expect={b1: -1, b2: -1})
    g["tie"] = [first, none]
    g["contention"] = [_contention(D, O)]
    g["node_sizes"] = [_node_size(D, O, n) for n in (64, 65, 128, 129)]
    culled = (len(ROTATION_PLAN) - 1,)
    g["rotation"] = [_rotation_plan(D, O, "rotation", ROTATION_PLAN, True, culled), _rotation_plan(D, O, "rotation_off", ROTATION_PLAN, False, culled),
                     _rotation_plan(D, O, "tenth_10", _tenth(10), True, ()), _rotation_plan(D, O, "tenth_11", _tenth(11), True, (11,))]
    g["scan"] = [scan_case(orc, O, D)]
    g["empty"] = [_empty(D, O, k) for k in ("n0_kf", "n0_frame", "zero_kf", "zero_frame")]
    g["masks"] = _masks(D, O)
    return voc, g


def random_case(voc, O, seed, nnratio=0.75, masked=True, n_points=260):
    """Two views of one scene of triangulate_cases.py, a mask over the keyframe's features."""
    sc = tc.random_scene(voc, 160 + seed, n_points, 1)
    rng = np.random.default_rng(9800 + seed)
    k, f = sc["kf1"], sc["neighbours"][0]
    tc.attach_bow([k, f], O)
    return dict(name="random_%d_%g%s" % (seed, nnratio, "" if masked else "_no_mask"), kf=k, frame=f, nnratio=nnratio, check_orientation=seed % 2 == 0,
                levelsup=tc.LEVELSUP, zero=(), valid=(rng.random(len(k["kp"])) < 0.85).astype(np.uint8) if masked else None, want=None, expect={}, notes={})


def oracle_kf_frame(orc, case):
    """-> (match (NF,): the keyframe feature whose map point the frame feature receives, nmatches)"""
    k, f = case["kf"], case["frame"]
    valid = np.ones(len(k["kp"]), np.uint8) if case["valid"] is None else case["valid"]
    bk = dict(fv_node=k["fv"][0], fv_feature=k["fv"][1]); bf = dict(fv_node=f["fv"][0], fv_feature=f["fv"][1])
    m, nm = orc.search_by_bow(k["kp"], k["desc"].reshape(-1, 32), valid, bk, f["kp"], f["desc"].reshape(-1, 32), bf, case["nnratio"], case["check_orientation"])
    return m, nm


def numpy_kf_frame(case, mutant=None, valid=None):
    """SearchByBoW(KeyFrame*, Frame&, ...) restated: per shared node a distance matrix; the keyframe's rows in order; per row the
    nearest and second nearest among the frame columns not yet taken; accepted at bestDist1 <= 50 and (float)bestDist1 < nnratio *
    (float)bestDist2; then the three largest bins of the rotation histogram keep their matches.  valid: the mask row to use."""
    k, f = case["kf"], case["frame"]
    NK, NF = len(k["kp"]), len(f["kp"])
    v = case["valid"] if valid is None else valid
    v = np.ones(NK, bool) if v is None else np.asarray(v[:NK], bool)
    match = np.full(NF, -1, np.int32); bins = np.full(NF, -1, np.int64)
    ratio = F32(case["nnratio"])
    nk, fk = k["fv"]; nf, ff = f["fv"]
    for node in np.intersect1d(nk, nf):
        rk = fk[nk == node]; rf = ff[nf == node]
        free = np.ones(len(rf), bool)
        D = np.unpackbits(k["desc"].reshape(-1, 32)[rk][:, None, :] ^ f["desc"].reshape(-1, 32)[rf][None, :, :], axis=2).sum(2).astype(np.int64)
        for a, iK in enumerate(rk):
            if not v[iK]:
                continue
            cols = np.nonzero(free)[0] if mutant != "ignore_taken" else np.arange(len(rf))
            if not len(cols):
                continue
            d = D[a, cols]
            j = int(np.argmin(d)); d1 = int(d[j])
            rest = np.delete(d, j)
            if mutant == "second_best_includes_taken":
                rest = np.delete(D[a], cols[j])
            d2 = int(rest.min()) if len(rest) else 256
            if d1 >= 256:
                continue
            ok1 = d1 < TH_LOW if mutant == "th_low_exclusive" else d1 <= TH_LOW
            ok2 = F32(d1) <= ratio * F32(d2) if mutant == "ratio_le" else F32(d1) < ratio * F32(d2)
            if ok1 and ok2:
                iF = int(rf[cols[j]])
                match[iF] = iK; free[cols[j]] = False
                rot = F32(k["kp"]["angle"][iK]) - F32(f["kp"]["angle"][iF])
                if rot < 0:
                    rot = F32(rot + F32(360.0))
                x = F32(rot * (F32(1.0) / F32(HISTO)))
                b = int(np.rint(x)) if mutant == "round_half_even" else int(np.floor(np.float64(x) + 0.5))
                bins[iF] = 0 if b == HISTO else b
    if case["check_orientation"]:
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
        if mutant == "hist_first_two":
            i3 = -1
        match[(bins >= 0) & ~np.isin(bins, [i1, i2, i3])] = -1
    return match, int((match >= 0).sum())


def numpy_kf_frame_call(cases, mutant=None):
    """The pairs of one call.  mask_by_kf_slot: a keyframe that takes part in several pairs reads the mask row of its first pair."""
    out = []
    for c in cases:
        v = None
        if mutant == "mask_by_kf_slot":
            v = next(o["valid"] for o in cases if o["kf"] is c["kf"])
        out.append(numpy_kf_frame(c, None if mutant == "mask_by_kf_slot" else mutant, valid=v))
    return out


def same_matches(case, got, want, what=""):
    gm, gn = got; wm, wn = want
    assert len(gm) == len(wm), "%s %s: %d vs %d frame features" % (what, case["name"], len(gm), len(wm))
    bad = np.nonzero(np.asarray(gm) != np.asarray(wm))[0]
    if len(bad):
        named = {v: n for n, v in _named_frame_features(case).items()}
        i = int(bad[0])
        raise AssertionError("%s %s: frame feature %d (%s) holds %d, meant %d; %d features differ" % (what, case["name"], i, named.get(i, "unnamed"), gm[i], wm[i], len(bad)))
    assert gn == wn, "%s %s: nmatches %d vs %d" % (what, case["name"], gn, wn)


def _named_frame_features(case):
    out = {}
    for name, v in case.get("notes", {}).items():
        if isinstance(v, tuple) and len(v) == 2 and all(isinstance(x, (int, np.integer)) for x in v):
            out[name] = int(v[1])
    return out


def check_expect(case, match):
    for iF, iK in case["expect"].items():
        assert int(match[iF]) == iK, "%s: frame feature %d holds %d, built for %d" % (case["name"], iF, match[iF], iK)


def call_groups(cases, per_call=4):
    """Cases that can share one call (one nnratio, one orientation switch), at most per_call pairs each.  Cases without a mask get calls
    of their own, so that the call passes no mask table at all."""
    by = {}
    for c in cases:
        by.setdefault((c["nnratio"], bool(c["check_orientation"]), c["valid"] is None), []).append(c)
    return [g[i:i + per_call] for g in by.values() for i in range(0, len(g), per_call)]


# ---------------------------------------------------------------- the device side (tests marked gpu)
def workspace(fe, n_slots, voc, big=False):
    ws = tc.Workspace(fe, n_slots, voc, GEOM_BIG if big else tc.GEOM)
    ws.voc, ws.V0 = voc, None
    return ws


def close_workspace(ws):
    if ws.V0 is not None:
        ws.V0.close()
    ws.close()


def write_slots(ws, frames, slots):
    """Key points (where the frame has any) and descriptors of frame j over slot slots[j]; nothing is computed."""
    import torch
    for s, f in zip(slots, frames):
        d = np.ascontiguousarray(f["desc"], np.uint8).reshape(-1)
        n = len(d) // 32
        assert 0 <= s < ws.n and n <= ws.cap
        if n:
            k = f.get("kp")
            if k is not None:
                ws.kp[s, :k.nbytes] = torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda()
            ws.desc[s, :len(d)] = torch.from_numpy(d.copy()).cuda()
        ws.count[s] = n
    torch.cuda.synchronize()


def device_compute_bow(ws, V, frames, levelsup, slots=None):
    """Descriptor arrays `frames` over the slots, ONE compute_bow call on them -> [download_bow(slot)]."""
    slots = list(range(len(frames))) if slots is None else list(slots)
    write_slots(ws, [dict(desc=d) for d in frames], slots)
    ws.b.compute_bow(V, slots, levelsup)
    ws.b.sync()
    return [ws.b.download_bow(s) for s in slots]


def device_kf_frame(ws, cases, slots=None):
    """All cases in ONE search_by_bow call.  slots[q] = (keyframe slot, frame slot) of case q, by default (2q, 2q + 1); cases that share a
    keyframe object may share its slot.  ComputeBoW runs once per levelsup (and once with a weightless vocabulary for the sides a case
    wants empty).  -> [(match (NF,), nmatches)]"""
    import torch
    slots = [(2 * q, 2 * q + 1) for q in range(len(cases))] if slots is None else slots
    held, plan = {}, {}
    for c, (sk, sf) in zip(cases, slots):
        for side, s in (("kf", sk), ("frame", sf)):
            assert s not in held or held[s] is c[side], "two frames in one slot"
            if s not in held:
                held[s] = c[side]
                plan.setdefault((c["levelsup"], side in c["zero"]), []).append(s)
    write_slots(ws, [held[s] for s in held], list(held))
    for (levelsup, zero), ss in plan.items():
        if zero and ws.V0 is None:
            ws.V0 = ws.fe.Vocabulary.from_nodes(with_zero_weights(ws.voc))
        ws.b.compute_bow(ws.V0 if zero else ws.V, ss, levelsup)
    (ratio, ori), = set((c["nnratio"], bool(c["check_orientation"])) for c in cases)
    d_valid = None
    if any(c["valid"] is not None for c in cases):
        v = np.ones((len(cases), ws.cap), np.uint8)
        for q, c in enumerate(cases):
            if c["valid"] is not None:
                v[q, :len(c["valid"])] = c["valid"]
        d_valid = torch.from_numpy(v).cuda()
    ws.b.search_by_bow([s[0] for s in slots], [s[1] for s in slots], ratio, ori, d_kf_valid=d_valid.data_ptr() if d_valid is not None else None)
    out = []
    for q, c in enumerate(cases):
        match, pairs, nm = ws.b.download_matches(q)
        n = len(c["frame"]["kp"])
        out.append((match[:n].copy(), nm))
    del d_valid
    return out
