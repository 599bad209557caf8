"""CPU only: the crafted extractor images of tests/extract_cases.py on the oracle.  The oracle equals the from-the-definition
restatement (FAST score, NMS, per-cell retry, quadtree, IC_Angle moments, steered BRIEF), every named case is witnessed in the oracle's
output, and for every case that names a wrong twin the twin's result on that image differs.  One summary line per builder, equal to
profiles/extract_cases_summary.txt (python tests/test_extract_cases.py rewrites the file)."""
import os
from collections import namedtuple

import numpy as np
import pytest

import extract_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = os.path.join(ROOT, "profiles", "extract_cases_summary.txt")
Run = namedtuple("Run", "shot o kp desc levels")       # levels[l] = int rows (x, y, response) of level l's key points, in output order


def run_shot(orc, shot):
    o = orc.Extractor(*shot.params)
    kp, desc = o(shot.img)                               # an unsupported geometry raises: a failure, never a skip
    levels, at = [], 0
    for l in range(o.nlevels):
        k = kp[at:at + o.per_level[l]]; at += o.per_level[l]
        s = np.float64(o.scale[l]) if l else 1.0
        levels.append(np.stack([np.rint(k["x"] / s), np.rint(k["y"] / s), k["response"]], 1).astype(np.int32).reshape(-1, 3))
    return Run(shot, o, kp, desc, levels)


@pytest.fixture(scope="module")
def runs(orc):
    return {b: [run_shot(orc, s) for s in shots] for b, shots in E.build_all(orc).items()}


def oracle_candidates(orc, plane, ini, mn):
    """The oracle's own FAST leaf per cell window with the extractor's retry, in level coordinates."""
    out = []
    for x0, y0, x1, y1, _, _ in E.cell_grid(plane.shape[1], plane.shape[0]):
        r = orc.fast(plane[y0:y1, x0:x1], ini)
        if len(r) == 0:
            r = orc.fast(plane[y0:y1, x0:x1], mn)
        out += [(x + x0, y + y0, s) for x, y, s in r]
    return np.array(out, np.int32).reshape(-1, 3)


_detect_cache = {}


def detect(r, level, twin=None):
    key = (r.shot.img.tobytes(), r.shot.params[1:], level, twin)
    if key not in _detect_cache:
        per_cell = []
        plane = r.o.pyramid(level)[E.EDGE:-E.EDGE, E.EDGE:-E.EDGE]
        _detect_cache[key] = (E.detect(plane, r.shot.params[3], r.shot.params[4], twin, per_cell), per_cell)
    return _detect_cache[key]


def lookup(rows, xy):
    m = (rows[:, 0] == xy[0]) & (rows[:, 1] == xy[1])
    return int(rows[m][0, 2]) if m.any() else None


def check_restatement(orc, rs):
    for r in rs:
        o, (nf, scale, nl, ini, mn) = r.o, r.shot.params
        at = 0
        for l in range(nl):
            pad = o.pyramid(l)
            plane = pad[E.EDGE:-E.EDGE, E.EDGE:-E.EDGE]
            if l == 0:
                assert np.array_equal(plane, r.shot.img) and np.array_equal(pad, E.reflect_pad(r.shot.img)), r.shot.name
            c, _ = detect(r, l)
            assert np.array_equal(c, oracle_candidates(orc, plane, ini, mn)), "%s level %d: FAST / NMS / retry per cell" % (r.shot.name, l)
            assert len(c) == o.cand_per_level[l], "%s level %d: %d candidates restated, oracle %d" % (r.shot.name, l, len(c), o.cand_per_level[l])
            kept = E.quadtree(c, plane.shape[1], plane.shape[0], int(o.quota[l]))
            assert np.array_equal(kept, r.levels[l]), "%s level %d: quadtree keeps %d, oracle %d" % (r.shot.name, l, len(kept), len(r.levels[l]))
            blurred = o.blurred(l)
            for i, (x, y, _) in enumerate(r.levels[l]):
                k = r.kp[at + i]
                m01, m10 = E.moments(pad, x, y)
                assert np.float32(orc.fast_atan2(m01, m10)).tobytes() == k["angle"].tobytes(), "%s level %d key point %d: angle" % (r.shot.name, l, i)
                assert np.array_equal(E.describe(blurred, x, y, k["angle"]), r.desc[at + i]), "%s level %d key point %d: descriptor" % (r.shot.name, l, i)
                assert k["octave"] == l and k["size"] == np.float32(int(np.float32(31) * o.scale[l]))
            at += len(r.levels[l])


@pytest.mark.parametrize("builder", E.BUILDERS)
def test_oracle_equals_restatement(orc, runs, builder):
    check_restatement(orc, runs[builder])


def extractor_candidates(orc, r, l):
    """The FAST candidates of level l as the oracle's extractor shows them.  It exports their number and the key points it keeps: where the
    quadtree kept every candidate (its division ran until each node held one) the key points ARE the candidates, and the case is looked
    up in them.  DistributeOctTree ends early when a pass adds no node (all points of every divided node in one child), which a few
    images meet; there the candidates are those of the oracle's FAST leaf per cell with the retry, whose number the extractor confirms."""
    o = r.o
    if o.per_level[l] == o.cand_per_level[l]:
        return r.levels[l]
    c = oracle_candidates(orc, o.pyramid(l)[E.EDGE:-E.EDGE, E.EDGE:-E.EDGE], r.shot.params[3], r.shot.params[4])
    assert len(c) == o.cand_per_level[l] and all(lookup(c, k[:2]) == k[2] for k in r.levels[l]), r.shot.name
    return c


def witness(orc, r, case):
    """Asserts the claim of one named case on the oracle's output, and that the claim's twin rule (if any) gives another result."""
    o, claim, xy, l = r.o, case.claim, case.xy, case.level
    what = "%s: %s" % (r.shot.name, case.name)
    kind = claim[0]
    twin = claim[-1] if isinstance(claim[-1], str) and claim[-1] in E.TWINS else None
    if kind in ("cand", "no_cand", "kp"):
        want = claim[1] if kind != "no_cand" else None
        rows = r.levels[l] if kind == "kp" else extractor_candidates(orc, r, l)
        assert lookup(rows, xy) == want, "%s: the extractor has %r at %r" % (what, lookup(rows, xy), xy)
        c, _ = detect(r, l)
        assert lookup(c, xy) == want, "%s: restated candidate at %r is %r" % (what, xy, lookup(c, xy))
        if twin:
            assert lookup(detect(r, l, twin)[0], xy) != want, "%s: twin %s gives the same" % (what, twin)
    elif kind == "no_kp":
        assert lookup(r.levels[l], xy) is None, what
    elif kind == "ncand":
        assert o.cand_per_level[l] == claim[1], "%s: %r" % (what, o.cand_per_level)
    elif kind == "ncand_level":
        assert o.cand_per_level[claim[1][0]] == claim[1][1], "%s: %r" % (what, o.cand_per_level)
    elif kind == "per_level":
        assert o.per_level[l] == claim[1], "%s: %r" % (what, o.per_level)
    elif kind == "per_level_over":
        assert o.per_level[l] > claim[1] and o.per_level[l] > o.quota[l], "%s: %r quota %r" % (what, o.per_level, o.quota)
    elif kind == "over_quota":
        assert (o.per_level > o.quota).any(), "%s: %r quota %r" % (what, o.per_level, o.quota)
    elif kind == "cell_over":
        assert max(detect(r, l)[1]) > claim[1], "%s: busiest cell %d" % (what, max(detect(r, l)[1]))
    elif kind == "twin":                                 # the quadtree's pick on response ties
        c, _ = detect(r, l)
        H, W = r.shot.img.shape
        assert not np.array_equal(E.quadtree(c, W, H, int(o.quota[l]), claim[1]), r.levels[l]), "%s: twin %s gives the same" % (what, claim[1])
    elif kind in ("moments", "desc_tie", "reach"):
        m = claim[1] if kind == "moments" else claim[2] if kind == "reach" else claim[1]
        assert lookup(r.levels[l], xy) is not None, "%s: no key point at %r" % (what, xy)
        assert E.moments(E.reflect_pad(r.shot.img), *xy) == tuple(m), "%s: moments %r" % (what, E.moments(E.reflect_pad(r.shot.img), *xy))
        k = r.kp[:o.per_level[0]][(r.levels[0][:, 0] == xy[0]) & (r.levels[0][:, 1] == xy[1])][0]
        ang = orc.fast_atan2(*m)
        assert k["angle"] == np.float32(ang), what
        if tuple(m) == (0, 0):
            assert k["angle"] == 0.0
        if kind == "desc_tie":
            t, f = E.tap_coords(ang)
            tw, _ = E.tap_coords(ang, twin)
            assert (np.abs(f - np.floor(f)) == 0.5).any() and not np.array_equal(t, tw), "%s: no tap on .5" % what
            d = r.desc[:o.per_level[0]][(r.levels[0][:, 0] == xy[0]) & (r.levels[0][:, 1] == xy[1])][0]
            assert not np.array_equal(E.describe(o.blurred(0), xy[0], xy[1], ang, twin), d), "%s: twin %s gives the same" % (what, twin)
        if kind == "reach":
            assert E.reach(ang) == claim[1] == 18, "%s: reaches %d" % (what, E.reach(ang))
    elif kind == "angle_in":
        k = r.kp[:o.per_level[0]][(r.levels[0][:, 0] == xy[0]) & (r.levels[0][:, 1] == xy[1])][0]
        assert claim[1][0] < k["angle"] < claim[1][1], "%s: %r" % (what, k["angle"])
    elif kind == "desc_zero":
        sel = (r.levels[0][:, 0] == xy[0]) & (r.levels[0][:, 1] == xy[1])
        assert sel.any(), "%s: no key point" % what
        d, k = r.desc[:o.per_level[0]][sel][0], r.kp[:o.per_level[0]][sel][0]
        assert not d.any(), what
        assert E.describe(o.blurred(0), xy[0], xy[1], k["angle"], twin).all(), "%s: twin %s gives the same" % (what, twin)
    elif kind == "twin_desc":
        n = 0
        for (x, y, _), k, d in zip(r.levels[0], r.kp, r.desc):
            n += not np.array_equal(E.describe(o.blurred(0), x, y, k["angle"], twin), d)
        assert n > 0, "%s: twin %s gives the same on all %d key points" % (what, twin, len(r.levels[0]))
    elif kind == "empty":
        assert len(r.kp) == 0 and not o.cand_per_level.any(), what
    elif kind == "has_kp":
        assert len(r.kp) > 0, what
    elif kind in ("cell_count", "cell_some"):            # the extractor's candidates inside one cell's scanned area
        x0, y0, x1, y1 = E.scan_areas(r.shot.img.shape[1], r.shot.img.shape[0])[claim[1]]
        k = extractor_candidates(orc, r, l)
        n = int(((k[:, 0] >= x0) & (k[:, 0] < x1) & (k[:, 1] >= y0) & (k[:, 1] < y1)).sum())
        assert n == detect(r, l)[1][claim[1]], "%s: %d key points, %d restated" % (what, n, detect(r, l)[1][claim[1]])
        assert n == claim[2] if kind == "cell_count" else n > 0, "%s: %d" % (what, n)
    elif kind == "ramp":                                 # no corner; on every level monotone along the ramp and (to one grey value) constant across it
        assert len(r.kp) == 0 and not o.cand_per_level.any(), what
        for lv in range(o.nlevels):
            p = o.pyramid(lv)[E.EDGE:-E.EDGE, E.EDGE:-E.EDGE].astype(np.int32)
            p = p if claim[1] == "x" else p.T
            # the resize's vertical pass truncates its two products separately: equal rows may come out one grey value apart
            assert np.abs(p - p[:1]).max() <= 1 and (np.diff(p[0]) >= 0).all() and p[0, -1] - p[0, 0] >= 250, "%s: level %d" % (what, lv)
    elif kind == "pyr_path":                             # which pyramid kernel writes each level >= 1, and over which tile grid
        W, H = r.shot.img.shape[::-1]
        got = E.pyr_paths(W, H, r.shot.params[1], r.shot.params[2])
        assert [g[0] for g in got] == list(range(1, o.nlevels)), what
        for g, lv in zip(got, range(1, o.nlevels)):      # the restated level sizes are the oracle's
            assert (g[1], g[2]) == o.pyramid(lv).shape[::-1], "%s: level %d is %r" % (what, lv, o.pyramid(lv).shape)
        assert [g[3:] for g in got] == list(claim[1]), "%s: %r" % (what, got)
    elif kind == "tile_edge":
        got = E.pyr_paths(r.shot.img.shape[1], r.shot.img.shape[0], r.shot.params[1], r.shot.params[2])[0]
        assert (got[1] + E.PT_XSHIFT, got[2]) == tuple(claim[1]) == (o.pyramid(1).shape[1] + E.PT_XSHIFT, o.pyramid(1).shape[0]), "%s: %r" % (what, got)
    else:
        raise AssertionError("unknown claim %r" % (claim,))


@pytest.mark.parametrize("builder", E.BUILDERS)
def test_named_cases_witnessed(orc, runs, builder):
    n = 0
    for r in runs[builder]:
        assert r.shot.cases, r.shot.name
        for case in r.shot.cases:
            witness(orc, r, case)
            n += 1
    assert n > 0
    # every builder yields key points; only the shots built to be empty yield none
    for r in runs[builder]:
        if not any(c.claim[0] in ("empty", "ramp") for c in r.shot.cases) and not all(c.claim[0] == "no_cand" for c in r.shot.cases):
            assert len(r.kp) > 0, "%s yields no key point" % r.shot.name


def test_lattice_counts_are_the_documented_ones(runs):
    got = {r.shot.img.shape[::-1]: int(r.o.cand_per_level[0]) for r in runs["lattice"] if r.shot.name.count("/") == 1 and "generic" not in r.shot.name}
    assert got == E.LATTICE_COUNTS
    big = [r for r in runs["lattice"] if r.shot.name == "lattice/640x480"][0]
    assert len(E.brute_fast(big.shot.img, 20)) == 37564                       # FAST corners of the whole 640 x 480 lattice
    assert sorted(int(r.o.cand_per_level[0]) for r in runs["lattice"] if "M=" in r.shot.name) == [2047, 2048, 2049, 8191, 8192, 8193]


def test_small_quotas_are_the_documented_ones(runs):
    q = {r.shot.params[0]: r.o.quota.tolist() for r in runs["small_quota"]}
    assert q[1] == [0, 0, 0, 0, 0, 0, 0, 1] and q[50] == [11, 9, 8, 6, 5, 4, 4, 3]
    for r in runs["small_quota"]:
        if "texture" in r.shot.name:                                             # 4 * nIni on every level: one full pass runs before n >= N is tested
            assert (r.o.per_level == 16).all(), "%s: %r" % (r.shot.name, r.o.per_level)
        else:                                                                    # the lattice fades out of the top levels
            assert (r.o.per_level[:6] == 16).all() and r.o.per_level[7] == 0, "%s: %r" % (r.shot.name, r.o.per_level)


def load_fuzz():
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_extract", os.path.join(ROOT, "tools", "fuzz_extract.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


DEFAULT_DRAWS = [(398, 397, 1.25, 6, 732, 12, 8, 'mixed'), (384, 383, 1.7, 2, 321, 14, 4, 'mixed'), (1105, 308, 1.5, 2, 905, 19, 10, 'texture'),
                 (239, 181, 1.2, 1, 527, 12, 7, 'mixed'), (370, 369, 1.1, 6, 794, 8, 3, 'texture'), (971, 499, 1.7, 1, 1132, 22, 2, 'mixed'),
                 (1124, 221, 1.15, 5, 1194, 32, 2, 'noise'), (1210, 136, 1.4, 1, 1045, 35, 18, 'texture'), (866, 184, 1.4, 2, 967, 31, 30, 'mixed'),
                 (717, 224, 1.15, 3, 2432, 39, 20, 'mixed'), (412, 411, 1.1, 7, 333, 20, 20, 'texture'), (358, 357, 1.2, 3, 1056, 14, 14, 'texture'),
                 (455, 433, 1.5, 1, 1064, 26, 15, 'texture'), (589, 133, 1.25, 2, 1127, 13, 8, 'texture'), (790, 441, 2.0, 2, 496, 11, 5, 'mixed'),
                 (465, 464, 1.3, 7, 601, 24, 24, 'texture'), (434, 433, 1.2, 3, 1432, 31, 15, 'texture'), (814, 159, 1.5, 3, 800, 35, 16, 'mixed'),
                 (1305, 518, 2.0, 2, 116, 29, 6, 'mixed'), (762, 442, 1.15, 1, 1193, 26, 5, 'mixed')]


def test_default_fuzz_draws_unchanged():
    """The 20 draws of test_gpu_extract.test_randomised_configurations (seed 23), as tools/fuzz_extract.py drew them before it learnt --crafted."""
    m = load_fuzz()
    rng = np.random.default_rng(23)
    assert [m.draw(rng) for _ in range(20)] == DEFAULT_DRAWS


def test_crafted_fuzz_draws_on_the_oracle(orc):
    """The 8 crafted draws of test_gpu_extract_cases.test_crafted_fuzz_draws: supported by the oracle, equal to the restatement, nfeatures below 4 * nIni among them."""
    m = load_fuzz()
    rng = np.random.default_rng(E.FUZZ_SEED)
    rs = []
    for k in range(E.FUZZ_DRAWS):
        w, h, scale, levels, nf, ini, mn, kind = m.draw_crafted(rng)
        rs.append(run_shot(orc, E.Shot("fuzz %d %s" % (k, kind), m.crafted_image(w, h, kind, rng), (nf, scale, levels, ini, mn), [])))
    check_restatement(orc, rs)
    assert min(r.shot.params[0] for r in rs) < 4 and sum(len(r.kp) for r in rs) > 0


def summary_lines(runs):
    lines = []
    for b in E.BUILDERS:
        rs = runs[b]
        lines.append("%s: %d images, levels %s, %d key points, %d named cases" % (
            b, len(rs), "/".join(str(n) for n in sorted({r.shot.params[2] for r in rs})), sum(len(r.kp) for r in rs),
            sum(len(r.shot.cases) for r in rs)))
    return lines


def test_summary(runs):
    lines = summary_lines(runs)
    print("\n".join(lines))
    with open(SUMMARY) as f:
        assert f.read().splitlines() == lines, "profiles/extract_cases_summary.txt is stale: python tests/test_extract_cases.py"


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    _orc = graft.load_oracle()
    _runs = {b: [run_shot(_orc, s) for s in shots] for b, shots in E.build_all(_orc).items()}
    with open(SUMMARY, "w") as f:
        f.write("\n".join(summary_lines(_runs)) + "\n")
    print(open(SUMMARY).read(), end="")
