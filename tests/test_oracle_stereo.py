"""CPU tests of the crafted stereo cases (tests/stereo_cases.py) on the reporting oracle orc_stereo_matches_ex: the case list
reaches the branches of Frame::ComputeStereoMatches that it claims to reach, at every geometry, so that the byte equality the
GPU tests assert on the same arrays is an equality on those branches.  The generators decide the outcomes by construction;
a seed that reaches fewer is a generator bug."""
import numpy as np
import pytest

import stereo_cases as sc

GEOMS = list(sc.GEOMS)


@pytest.fixture(scope="module")
def suites(orc):
    memo = {}

    def get(name):
        if name not in memo:
            cases = sc.suite(sc.GEOMS[name])
            memo[name] = {c["name"].split("/")[1]: (c, sc.oracle(orc, c)) for c in cases}
        return memo[name]
    return get


def _hamming(a, b):
    return np.unpackbits(a ^ b, axis=-1).sum(-1)


@pytest.mark.parametrize("name", GEOMS)
def test_geometry_tables_are_the_extractors(orc, name):
    """The f32 tables and level sizes that the generators place key points with are the oracle extractor's own."""
    g = sc.GEOMS[name]
    e = orc.Extractor(*g.extractor_args())
    assert e.scale.tobytes() == g.scale.tobytes() and e.inv_scale.tobytes() == g.inv.tobytes()
    e(sc.images(g, "flat", 0)[0])
    for l in range(g.n_levels):
        assert e.pyramid(l).shape == (g.lh[l] + 38, g.lw[l] + 38)
    assert sc.SR_ROWS + 2 * g.band_r + 2 <= 96, "the geometry must fit the staged row slice"
    assert sc.SR_ROWS + 2 * sc.REFUSED.band_r + 2 > 96, "the refused geometry must not"
    assert sc.KP_DTYPE == orc.KP_DTYPE and sc.KP_DTYPE.itemsize == 28


def test_widest_accepted_band():
    assert sc.GEOMS["1280x1008-5x2.0"].band_r == 34 and sc.GEOMS["1024x500-12x1.2"].n_levels == 12
    assert sc.GEOMS["752x240-8x1.2"].H % 16 == 0 and sc.GEOMS["1241x376-8x1.2"].H % 16 != 0


@pytest.mark.parametrize("name", GEOMS)
def test_every_outcome_is_reached(orc, suites, name):
    h = sc.histogram([r for _, r in suites(name).values()])
    for code in (orc.ST_NO_CANDIDATE, orc.ST_HAMMING, orc.ST_WINDOW, orc.ST_EDGE_SHIFT, orc.ST_DISPARITY, orc.ST_CLAMPED,
                 orc.ST_MATCHED, orc.ST_REMOVED):
        assert h[code] >= 8, "%s: outcome '%s' reached by %d key points" % (name, orc.ST_NAMES[code], h[code])
    # maxU = uL >= 0 inside the domain.  deltaR: the chosen shift is the first strict minimum, so dist1 > dist2 and dist3 >= dist2,
    # hence |dist1 - dist3| <= dist1 + dist3 - 2 dist2 and |deltaR| <= 0.5: both exits stay in kernel and oracle
    # because the reference has them, and no input reaches them.
    assert h[orc.ST_MAXU_NEGATIVE] == 0 and h[orc.ST_DELTA] == 0


@pytest.mark.parametrize("name", GEOMS)
def test_cases_reach_what_they_are_named_for(orc, suites, name):
    S = suites(name)
    g = sc.GEOMS[name]
    out = lambda k: np.bincount(S[k][1]["outcome"], minlength=10)
    # exact copies: median 0, thDist 0, every match removed
    for k in ("exact_copy-d0", "exact_copy-d9"):
        r = S[k][1]
        assert r["nm"] >= 50 and r["median"] == 0 and r["th_dist"] == 0 and (r["ur"] == -1).all() and out(k)[orc.ST_MATCHED] == 0
        assert out(k)[orc.ST_REMOVED] == r["nm"]
    # Hamming thresholds: 74 passes, 75 / 99 / 100 do not (100 is not even a candidate: bestDist starts at TH_HIGH)
    r = S["hamming_thresholds"][1]
    assert r["hamming"].tolist() == [74] * 12 + [75] * 12 + [99] * 12 + [100] * 12
    assert (r["outcome"][:12] >= orc.ST_WINDOW).all() and (r["sad"][:12] >= 0).sum() >= 8
    assert (r["outcome"][12:] == orc.ST_HAMMING).all() and (r["best_idx"][36:] == -1).all() and (r["best_idx"][12:36] >= 0).all()
    # ties of 2 .. 5 in every order: the lowest right index of the group wins
    c, r = S["hamming_ties"]
    assert np.bincount(r["ties"]).tolist() == [0, 0, 2, 6, 24, 120]
    first = np.concatenate([[0], np.cumsum(r["ties"])[:-1]])
    assert np.array_equal(r["best_idx"], first) and (r["hamming"] == 30).all()
    winners_x = c["kL"]["x"] - c["kR"]["x"][r["best_idx"]]
    assert len(np.unique(winners_x)) == 5, "the winner must be the true partner in some groups and every other member in others"
    # octave gate: the nearer descriptor (10 bits) sits on a forbidden level, the winner is 40 bits away
    r = S["octave_gate"][1]
    assert (r["hamming"] == 40).all() and (r["ties"] == 1).all()
    lv = S["octave_gate"][0]["kL"]["octave"]
    assert {0, g.n_levels // 2, g.n_levels - 1} == set(lv.tolist())
    # u range: on the limit admitted (and matched), one ulp beyond it not
    r = S["u_range-hi"][1]
    assert (r["outcome"][:10] == orc.ST_MATCHED).all() and (r["best_idx"][10:20] == -1).all() and (r["outcome"][20:] == orc.ST_MATCHED).all()
    cL = S["u_range-hi"][0]["kL"]
    assert (cL["x"][20:] < g.maxD).all(), "minU < 0"
    r = S["u_range-lo"][1]
    assert (r["outcome"][:10] == orc.ST_MATCHED).all() and (r["best_idx"][10:] == -1).all()
    for k in ("refine_out_of_range-hi", "refine_out_of_range-lo"):
        assert (S[k][1]["outcome"] == orc.ST_DISPARITY).all()
    # window: column Wl - 11 refused at every level, 0 and Wl - 12 accepted; best shifts on and beside the edge
    c, r = S["window_edges"]
    n = 24 * g.n_levels
    o = r["outcome"][:n].reshape(g.n_levels, 3, 8)
    assert (o[:, 2] == orc.ST_WINDOW).all() and (o[:, :2] != orc.ST_WINDOW).all()
    sh = r["shift"][n:].reshape(4, 10)
    assert (sh[0] == 5).all() and (sh[1] == -5).all() and (sh[2] == 4).all() and (sh[3] == -4).all()
    assert (r["outcome"][n:n + 20] == orc.ST_EDGE_SHIFT).all() and (r["outcome"][n + 20:] >= orc.ST_CLAMPED).all()
    r = S["window_edges-flat"][1]
    assert (r["shift"] == -5).all() and (r["outcome"] == orc.ST_EDGE_SHIFT).all()
    assert S["window_edges-binary"][1]["sad"].max() > 255 * 4, "0 / 255 texture: large SADs even at the best shift"
    # the filter: match counts 0, 1, 2, 3, even, odd; the median inside a run; both sides of thDist in one frame
    for n_ in sc.FILTER_COUNTS:
        assert S["filter_counts-n%d" % n_][1]["nm"] == n_
    r = S["filter_counts-duplicates"][1]
    assert r["nm"] == 21 and (r["sad"][5:] == r["median"]).all() and (r["outcome"][5:] == orc.ST_MATCHED).all()
    k = "filter_counts-loud"
    assert out(k)[orc.ST_MATCHED] >= 8 and out(k)[orc.ST_REMOVED] >= 8
    # counts
    assert [len(S[k][0]["kL"]) for k in S if k.startswith("counts-")] == [0, 50, 0, 1, g.cap - 1, g.cap, g.cap, 1]
    assert S["counts-50x0"][1]["nm"] == 0 and S["counts-%dx%d" % (g.cap, g.cap)][1]["nm"] > g.cap // 2
    for d in sc.SHIFTS:
        assert S["shifted-d%d" % d][1]["nm"] >= 50


@pytest.mark.parametrize("name", GEOMS)
def test_zero_disparity_is_clamped(orc, suites, name):
    """Key points on the axis of a mirror-symmetric strip that both eyes see unshifted: dist1 == dist3, deltaR == 0, bestuR == uL
    bit for bit, disparity 0 -> 0.01 with the f64 uL - 0.01; their SAD of 0 survives the median of the frame."""
    c, r = suites(name)["zero_disparity"]
    g = sc.GEOMS[name]
    col = sc.zero_disparity_column(g)
    assert (r["outcome"][:40] == orc.ST_CLAMPED).all() and (r["outcome"][40:] != orc.ST_CLAMPED).all()
    assert (r["dep"][:40] == np.float32(g.bf) / np.float32(0.01)).all()
    assert (r["ur"][:40] == np.float32(np.float64(col) - 0.01)).all() and (r["sad"][:40] == 0).all() and r["median"] > 0
    # the test fails when the generator stops reaching the branch: half a column off the axis nothing is clamped
    broken = sc.zero_disparity(g, offset=0.5)
    assert (sc.oracle(orc, broken)["outcome"] != orc.ST_CLAMPED).all()


@pytest.mark.parametrize("name", GEOMS)
def test_ties_across_candidate_passes_and_left_passes(orc, suites, name):
    """The tied candidates lie on different rows with more than 256 other right key points on the rows strictly between them: the
    row-sorted staging order of k_stereo_match puts them into different 256-candidate passes, whatever the (undefined) order
    inside a row.  One 16-row chunk holds more than two passes of 128 left key points."""
    S = suites(name)
    for low in ("low", "high"):
        c, r = S["hamming_passes-" + low]
        rows = c["kR"]["y"].astype(np.int64)
        assert (r["ties"] == 2).all() and np.array_equal(r["best_idx"], np.arange(8))
        for i in range(len(c["kL"])):
            tied = np.nonzero(_hamming(c["dR"], c["dL"][i]) == r["hamming"][i])[0]
            assert len(tied) == 2 and tied[0] == r["best_idx"][i]
            lo, hi = sorted(rows[tied])
            assert ((rows > lo) & (rows < hi)).sum() > sc.SR_CAND
            assert (rows[tied[0]] < rows[tied[1]]) == (low == "low")
            assert lo // sc.SR_ROWS == hi // sc.SR_ROWS == int(c["kL"]["y"][i]) // sc.SR_ROWS
    c, r = S["left_passes"]
    chunk = np.bincount(c["kL"]["y"].astype(np.int64) // sc.SR_ROWS)
    assert chunk.max() > 2 * sc.SR_LEFT and r["nm"] > 2 * sc.SR_LEFT


@pytest.mark.parametrize("name", GEOMS)
def test_row_band_limits(orc, suites, name):
    """Every right key point of the row_band case is its left key point's only candidate: admitted exactly when the f32 band test
    says so, on both sides of both limits, for every octave, and at the distance from the key point's own row that the
    kernel's pre-filter band = ceil(rmax) + 1 has to cover (ceil(rmax) alone would not)."""
    c, r = suites(name)["row_band"]
    g = sc.GEOMS[name]
    yi = c["kL"]["y"].astype(np.int64)
    inside = np.array([sc._in_band(y, np.float32(2.0) * g.scale[o], row) for y, o, row in zip(c["kR"]["y"], c["kR"]["octave"], yi)])
    # (an unrelated descriptor is under TH_HIGH = 100 bits once in a few thousand pairs: the question is whether the partner won)
    assert np.array_equal(r["best_idx"] == np.arange(len(yi)), inside) and (r["hamming"][inside] == 20).all()
    assert set(c["kR"]["octave"].tolist()) == set(range(g.n_levels))
    last = (g.H - 1) // sc.SR_ROWS * sc.SR_ROWS
    assert {0, 15, 16, last, g.H - 1} == set(yi.tolist())
    rmax = np.float32(2.0) * g.scale[np.minimum(c["kL"]["octave"] + 1, g.n_levels - 1)]
    reach = yi - c["kR"]["y"].astype(np.int64)                        # rows between the left row and the candidate's own row
    tight = inside & (reach == np.ceil(rmax).astype(np.int64) + 1)
    assert tight.sum() >= 8 and (r["sad"][tight] >= 0).sum() >= 4, "candidates that only band = ceil(rmax) + 1 still scans"
    assert not (inside & (np.abs(reach) > np.ceil(rmax) + 1)).any()
    fr = c["kR"]["y"] - np.floor(c["kR"]["y"])
    assert (fr == 0).sum() >= 8 and ((fr > 0.998) & (fr < 1)).sum() >= 8


def test_ex_and_plain_entry_agree_on_the_golden_pair(orc, synth):
    cfg = synth.KITTI_STEREO
    L, R, _ = synth.stereo_frame(seq=7, t=0)
    eL = orc.Extractor(2000, 1.2, 8, 12, 7); eR = orc.Extractor(2000, 1.2, 8, 12, 7)
    kL, dL = eL(L); kR, dR = eR(R)
    ur, dep, sad, nm = orc.stereo_matches(eL, eR, kL, dL, kR, dR, cfg["bf"], cfg["fx"])
    r = orc.stereo_matches_ex(eL, eR, kL, dL, kR, dR, cfg["bf"], cfg["fx"])
    assert nm == r["nm"] and ur.tobytes() == r["ur"].tobytes() and dep.tobytes() == r["dep"].tobytes() and sad.tobytes() == r["sad"].tobytes()
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_kitti.npz"))
    assert nm == int(g["nmatched"]) and np.array_equal(r["sad"], g["sad"]) and r["ur"].tobytes() == g["uright"].tobytes()
    kept = r["outcome"] >= orc.ST_CLAMPED
    assert np.array_equal(kept, r["sad"] >= 0) and np.array_equal(r["outcome"] == orc.ST_REMOVED, (r["sad"] >= 0) & (r["ur"] < 0))
    assert r["median"] == np.sort(r["sad"][r["sad"] >= 0])[nm // 2] and r["th_dist"] == np.float32(1.5) * np.float32(1.4) * np.float32(r["median"])


def test_domain_check_refuses_what_the_kernel_must_not_see():
    g = sc.GEOMS["752x240-8x1.2"]
    good = sc.filter_count(g, 3)
    for field, value in (("x", -0.5), ("x", g.W), ("y", g.H), ("y", np.nan), ("x", np.inf), ("octave", g.n_levels), ("octave", -1)):
        bad = dict(good, kR=good["kR"].copy())
        bad["kR"][field][1] = value
        with pytest.raises(AssertionError):
            sc.check_domain(bad)
    with pytest.raises(AssertionError):
        sc.check_domain(sc.counts(g, g.cap, g.cap), g.cap - 1)
