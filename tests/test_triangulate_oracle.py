"""The CreateNewMapPoints CPU oracle (tests/cpp/triangulate_oracle.cpp) on the crafted cases of triangulate_cases.py: which branch
every case reaches is pinned here (a named branch reached by no case fails), the thresholds are scanned in 1-ulp steps, the frozen
null vector is held against numpy's SVD, and the device's reformulation (independent pairs, then the first surviving neighbour per
idx1) is shown to equal the sequential loop.  The GPU tests (test_gpu_triangulate.py) compare the device with this oracle byte
for byte on the same cases.

Contraction: the oracle built with -ffp-contract=fast (and FMA) decides 745 of the 2,560 scan points below differently (9 on the epipolar
bound, 32 / 192 on the mono and 256 / 256 on the stereo reprojection bounds of KF1 / KF2; test_threshold_scans_see_contraction recounts
them and asserts that every bound has some), so a contracted device build
does not pass the GPU suite unnoticed.

`x3D[3] == 0` (LocalMapping.cc:334) is reached by no rigid pair of poses (rays with parallax never meet at infinity), but the call
takes any 4x4 matrix: the case `nonrigid_w0` reaches it with Rcw = diag(0, 1, 1)."""
import numpy as np
import pytest

import triangulate_cases as tc

F32 = np.float32


@pytest.fixture(scope="module")
def matcher(synth, orc):
    voc, cases = tc.matcher_cases(synth)
    O = orc.Vocabulary.from_nodes(voc)
    for c in cases:
        tc.attach_bow([c["kf1"]] + c["neighbours"], O)
    return {c["name"]: c for c in cases}


@pytest.fixture(scope="module")
def creation(synth, orc):
    voc, cases = tc.creation_cases(synth)
    O = orc.Vocabulary.from_nodes(voc)
    for c in cases:
        tc.attach_bow([c["kf1"]] + c["neighbours"], O)
    return {c["name"]: c for c in cases}


def test_cases_are_what_they_claim(matcher, creation):
    """Node membership and descriptor distances of every crafted case are the chosen ones."""
    for c in list(matcher.values()) + list(creation.values()):
        for kf2, want in zip(c["neighbours"], c["want"]):
            tc.check_distances(c["kf1"], kf2, want)


def test_matcher_branches(matcher):
    c = matcher["all"]; n = c["notes"]
    kf1, kf2 = c["kf1"], c["neighbours"][0]
    r = tc.search(kf1, kf2)
    m, br = r["match"], r["branches"]
    for (i1, i2) in n["plain"]:
        assert m[i1] == i2
    assert m[n["d50"][0]] == n["d50"][1] and br["best50"] == 1, "dist = 50 is accepted"
    assert m[n["d51"][0]] == -1 and br["dist51"] >= 1, "dist = 51 is rejected"
    assert m[n["tie"][0]] == n["tie"][2] and n["tie"][2] > n["tie"][1] and br["tie_later_wins"] >= 1, "equal distance: the later feature wins"
    for order in (0, 1):
        i1, i2 = n["better_fails_%d" % order]
        assert m[i1] == i2, "the candidate on the epipolar line wins although the other is closer"
    assert br["better_failed_worse_passed"] == 2 and br["epi_fail"] >= 2
    assert m[n["epipole_mono"][0]] == -1 and br["epipole_excluded"] == 1, "mono-mono next to the epipole is excluded"
    assert m[n["epipole_stereo1"][0]] == n["epipole_stereo1"][1] and br["epipole_near_but_stereo"] == 1, "... and only mono-mono"
    assert m[n["has_mp1"][0]] == -1 and br["skip_mp1"] == 1
    assert m[n["has_mp2"][0]] == n["has_mp2"][2] and br["skip_mp2"] >= 1
    a, b, i2 = n["shared_idx2"]
    assert m[a] == i2 and m[b] == i2 and br["two_idx1_one_idx2"] == 1, "vbMatched2 is never set: two idx1 take one idx2"
    assert m[n["big_node"][0]] == n["big_node"][1] and br["big_node"] == 1, "a node beyond the register path"
    for (i1, i2) in n["rot90"]:
        assert m[i1] == i2
    assert br["hist_culled"] == 0 and br["den_zero"] == 0
    assert r["nmatches"] == len(r["pairs"]) == int((m >= 0).sum())
    assert np.array_equal(r["pairs"][:, 0], np.nonzero(m >= 0)[0]) and np.array_equal(r["pairs"][:, 1], m[m >= 0])
    # the rotation histogram on: the match that turns by 90 degrees goes
    h = tc.search(kf1, kf2, check_orientation=True)
    assert h["branches"]["hist_culled"] == 1 and h["nmatches"] == r["nmatches"] - 1
    for (i1, _) in n["rot90"]:
        assert h["match"][i1] == -1
    # bOnlyStereo: monocular features leave on both sides
    s = tc.search(kf1, kf2, only_stereo=True)
    assert s["branches"]["skip_onlystereo1"] > 0 and s["branches"]["skip_onlystereo2"] > 0
    st1, st2 = kf1["ur"] >= 0, kf2["ur"] >= 0
    assert 0 < s["nmatches"] < r["nmatches"] and all(st1[i] and st2[j] for i, j in s["pairs"])


def test_matcher_small_and_degenerate(matcher):
    r = tc.search(matcher["identical_poses"]["kf1"], matcher["identical_poses"]["neighbours"][0])
    assert not r["F12"].any() and r["nmatches"] == 0 and r["branches"]["den_zero"] > 0, "identical poses: F12 = 0, den == 0"
    for name in ("empty1", "empty2"):
        r = tc.search(matcher[name]["kf1"], matcher[name]["neighbours"][0])
        assert r["nmatches"] == 0 and r["branches"]["shared_node"] == 0
    r = tc.search(matcher["single"]["kf1"], matcher["single"]["neighbours"][0])
    assert r["nmatches"] == 1 and r["match"].tolist() == [0]
    r = tc.search(matcher["no_shared_node"]["kf1"], matcher["no_shared_node"]["neighbours"][0])
    assert r["nmatches"] == 0 and r["branches"]["shared_node"] == 0


EXPECT = {   # name -> (path, outcome, stereo1, stereo2)
    "svd_mono_mono": ("svd", "created", 0, 0), "svd_stereo_mono": ("svd", "created", 1, 0), "svd_mono_stereo": ("svd", "created", 0, 1),
    "svd_both_stereo": ("svd", "created", 1, 1), "mono_mono_parallel": ("none", "low_parallax", 0, 0), "z1_negative": ("svd", "z1", 0, 0),
    "reproj1_mono": ("svd", "reproj1_mono", 0, 0), "reproj1_stereo": ("svd", "reproj1_stereo", 1, 0), "created_off_line": ("svd", "created", 0, 0),
    "reproj2_stereo_svd": ("svd", "reproj2_stereo", 0, 1), "scale_low": ("svd", "scale_low", 0, 0), "scale_high": ("svd", "scale_high", 0, 0),
    "unproject1": ("unproject1", "created", 1, 0), "unproject2": ("unproject2", "created", 0, 1),
    "quirk_both_stereo": ("unproject1", "created", 1, 1), "reproj2_mono": ("unproject1", "reproj2_mono", 1, 0),
    "reproj2_stereo": ("unproject1", "reproj2_stereo", 1, 1), "reproj1_mono_unproject2": ("unproject2", "reproj1_mono", 0, 1),
    "z2_negative": ("svd", "z2", 0, 0), "cos_negative": ("none", "low_parallax", 0, 0), "created_then_absent": ("svd", "created", 0, 0),
    "rejected_then_created": ("svd", "z1", 0, 0), "no_depth": ("unproject1", "no_depth", 1, 0),
}


def test_triangulation_branches(creation):
    c = creation["branches"]
    r = tc.create(c["kf1"], c["neighbours"])
    tr = {(int(t["neighbour"]), int(t["idx1"])): t for t in r["trace"]}
    assert set(c["notes"]) == set(EXPECT)
    for name, (nb, i1) in c["notes"].items():
        t = tr[(nb, i1)]
        got = (tc.PATHS[t["path"]], tc.OUTCOMES[t["outcome"]], int(t["stereo1"]), int(t["stereo2"]))
        assert got == EXPECT[name], "%s: %r, cos %r" % (name, got, t["cosRays"])
    t = tr[c["notes"]["mono_mono_parallel"]]; assert 0.9998 <= t["cosRays"] < 1
    t = tr[c["notes"]["cos_negative"]]; assert t["cosRays"] <= 0
    # every named outcome and path is reached: w0 by the case of its own, dist0 (x3D exactly on a camera centre) by none
    w = creation["nonrigid_w0"]
    rw = tc.create(w["kf1"], w["neighbours"])
    assert len(rw["trace"]) == 2 and len(rw["new"]) == 0
    for t in rw["trace"]:
        assert (tc.PATHS[t["path"]], tc.OUTCOMES[t["outcome"]]) == ("svd", "w0") and 0 < t["cosRays"] < 0.9998 and not t["A"].reshape(4, 4)[:, 0].any()
    seen_o = {tc.OUTCOMES[t["outcome"]] for t in list(r["trace"]) + list(rw["trace"])}; seen_p = {tc.PATHS[t["path"]] for t in r["trace"]}
    assert seen_o == set(tc.OUTCOMES) - {"dist0"} and seen_p == set(tc.PATHS)
    # the neighbour loop
    nb, i1 = c["notes"]["created_then_absent"]
    assert (1, i1) not in tr and (0, i1) in tr, "created at neighbour 0: neighbour 1 never matches it"
    nb, i1 = c["notes"]["rejected_then_created"]
    assert tc.OUTCOMES[tr[(1, i1)]["outcome"]] == "created", "rejected at neighbour 0, created at neighbour 1"
    new = r["new"]
    assert len(new) == sum(tc.OUTCOMES[t["outcome"]] == "created" for t in r["trace"])
    key = new["neighbour"].astype(np.int64) * 100000 + new["idx1"]
    assert np.all(np.diff(key) > 0), "creation order: neighbour ascending, then idx1"


def test_unproject_reads_the_raw_key_points(creation):
    """mvKeys and mvKeysUn differ by 1.5 px: the unprojected point comes from mvKeys (KeyFrame.cc:620-621), on either side."""
    c = creation["raw_keys"]
    r = tc.create(c["kf1"], c["neighbours"])
    assert [tc.PATHS[t["path"]] for t in r["trace"]] == ["unproject1", "unproject2"] and len(r["new"]) == 2
    fx, fy, cx, cy = [float(tc.CAM[k]) for k in ("fx", "fy", "cx", "cy")]
    for name, rec in zip(("unproject1", "unproject2"), r["new"]):
        i1, T, (u, v), z = c["notes"][name]
        assert rec["idx1"] == i1
        from_raw = tc.to_world(T, [(u - cx) * z / fx, (v - cy) * z / fy, z])[0]
        kf = c["kf1"] if name == "unproject1" else c["neighbours"][0]
        k = kf["kp"][rec["idx1"] if name == "unproject1" else rec["idx2"]]
        from_un = tc.to_world(T, [(float(k["x"]) - cx) * z / fx, (float(k["y"]) - cy) * z / fy, z])[0]
        assert np.abs(rec["xw"] - from_raw).max() < 1e-4 and np.abs(rec["xw"] - from_un).max() > 0.02, name


def test_neighbour_rules(creation):
    r = tc.create(creation["zero_neighbours"]["kf1"], [])
    assert len(r["new"]) == 0 and len(r["trace"]) == 0
    c = creation["stereo_rule"]
    r = tc.create(c["kf1"], c["neighbours"])
    assert r["branches"]["neigh_skip_stereo"] == 1 and r["branches"]["neigh_run"] == 1 and r["new"]["neighbour"].tolist() == [1]
    c = creation["mono_rule"]
    r = tc.create(c["kf1"], c["neighbours"], c["median_depth"])
    assert r["branches"]["neigh_skip_mono"] == 1 and r["branches"]["neigh_run"] == 1 and r["new"]["neighbour"].tolist() == [1]


def _alone(c, k, lv=None):
    """Neighbour k run alone against the keyframe's initial map points."""
    md = None if c["median_depth"] is None else [c["median_depth"][k]]
    return tc.create(c["kf1"], [c["neighbours"][k]], md, lv=lv)["new"]


def test_first_surviving_neighbour_equals_the_sequential_loop(creation, synth, orc):
    """The device's decomposition: every (keyframe, neighbour) pair on its own, then the first surviving neighbour per idx1."""
    cases = list(creation.values())
    voc = tc.vocabulary(synth, 6)
    O = orc.Vocabulary.from_nodes(voc)
    for seed, n, k, median in ((1, 150, 4, False), (2, 120, 6, True)):
        c = tc.random_scene(voc, seed, n, k, median=median)
        tc.attach_bow([c["kf1"]] + c["neighbours"], O)
        cases.append(c)
    total = 0
    for c in cases:
        seq = tc.create(c["kf1"], c["neighbours"], c["median_depth"])["new"]
        par = tc.first_surviving([_alone(c, k) for k in range(len(c["neighbours"]))])
        assert seq.tobytes() == par.tobytes(), c["name"]
        total += len(seq)
    assert total > 100


def _svd_reference(A):
    """x3D from numpy's SVD in float64 of the same f32 A."""
    v = np.linalg.svd(A.astype(np.float64).reshape(4, 4))[2][3]
    return v[:3] / v[3]


def test_null_vector_accuracy(creation, synth, orc):
    """The frozen Jacobi null vector against numpy.linalg.svd (float64) of the same A: 1e-5 * max(1, |x|) per coordinate, the
    project's 1e-5 bar, on the SVD-branch matches with at least 1 degree of parallax."""
    voc = tc.vocabulary(synth, 6)
    O = orc.Vocabulary.from_nodes(voc)
    traces = [tc.create(creation["branches"]["kf1"], creation["branches"]["neighbours"])["trace"]]
    for seed in (3, 4):
        c = tc.random_scene(voc, seed, 200, 4, noise=0.5)
        tc.attach_bow([c["kf1"]] + c["neighbours"], O)
        traces.append(tc.create(c["kf1"], c["neighbours"])["trace"])
    n = 0; worst = 0.0
    for t in np.concatenate(traces):
        if tc.PATHS[t["path"]] != "svd" or tc.OUTCOMES[t["outcome"]] == "w0" or t["cosRays"] > np.cos(np.deg2rad(1.0)):
            continue
        ref = _svd_reference(t["A"])
        err = np.abs(t["x3D"].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max())); n += 1
        assert np.all(err <= 1e-5), "x3D %r vs %r" % (t["x3D"], ref)
    print("null vector: %d matrices, worst relative error %.3g" % (n, worst))
    assert n > 100


def test_null_vector_sweeps_converged():
    """8 sweeps is past convergence: 12 sweeps give the same f32 vector bit for bit, 6 sweeps the same to 2e-7, on ill- and well-conditioned inputs."""
    rng = np.random.default_rng(11)
    for i in range(200):
        A = rng.normal(size=(4, 4)).astype(F32) * F32(10.0 ** rng.integers(-2, 3))
        if i % 4 == 0:
            A[3] = A[2] * F32(1 + 1e-4) + F32(1e-5) * rng.normal(size=4).astype(F32)      # two nearly dependent rows
        x8, _ = tc.null4(A)
        x6, _ = tc.null4(A, sweeps=6)
        x12, _ = tc.null4(A, sweeps=12)
        assert x8.tobytes() == x12.tobytes(), i
        assert np.allclose(x6, x8, rtol=0, atol=2e-7), i


def test_null_vector_w_zero():
    """A zero first column: every pair with it has gamma == 0 (no rotation), its norm 0 is the smallest: the vector is e0, w == 0."""
    A = np.array([[0, 1, 2, 3], [0, -1, 0.5, 2], [0, 3, 1, -1], [0, 0.2, -2, 1]], F32)
    x, v = tc.null4(A)
    assert x.tolist() == [1.0, 0.0, 0.0, 0.0] and x[3] == 0
    # ties: the first column of the smallest norm wins
    x, _ = tc.null4(np.diag([2, 1, 1, 3]).astype(F32))
    assert x.tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.fixture(scope="module")
def scans(synth, orc):
    voc = tc.vocabulary(synth, 6)
    O = orc.Vocabulary.from_nodes(voc)
    return {kind: tc.scan_case(voc, O, kind, 512) for kind in tc.SCAN_KINDS}


def test_threshold_scans(scans):
    """The sliding coordinate (see triangulate_cases._scan_rows) crosses 3.84 sigma^2 (CheckDistEpipolarLine), 5.991 sigma^2 (mono
    reprojection, either camera) and 7.8 sigma^2 (stereo reprojection, either camera) in 1-ulp steps: every scan holds both outcomes
    and nothing but the named rejection."""
    for kind, c in scans.items():
        kf1, kf2 = c["kf1"], c["neighbours"][0]
        off = tc.scan_accepted(kind, kf1, kf2)
        assert len(off) == 512 and off.any() and not off.all(), "%s: the scan must hold both outcomes" % kind
        if kind != "epipolar":
            out = {tc.OUTCOMES[t["outcome"]] for t in tc.create(kf1, [kf2])["trace"]}
            assert out == {"created", kind}, out


def test_threshold_scans_see_contraction(scans):
    """The same scans through an oracle built with -ffp-contract=fast: the decisions that differ are what the GPU suite would notice of
    a contracted device build.  When written: 2,560 scan points, 745 decisions differ, at least 9 on every bound."""
    if not tc.host_has_fma():
        pytest.skip("the host CPU has no FMA: a contracted build cannot run here")
    changed = 0; points = 0
    for kind, c in scans.items():
        kf1, kf2 = c["kf1"], c["neighbours"][0]
        off, fast = tc.scan_accepted(kind, kf1, kf2), tc.scan_accepted(kind, kf1, kf2, contract="fast")
        assert (off != fast).any(), "%s: no scan decision changes under contraction: densify the scan" % kind
        changed += int((off != fast).sum()); points += len(off)
        print("%s: %d of %d accepted, %d decisions differ under contraction" % (kind, off.sum(), len(off), (off != fast).sum()))
    print("contraction changes %d of %d scan decisions" % (changed, points))
    assert points == 2560
    assert changed > 0, "no scan decision changes under contraction: densify the scans"
