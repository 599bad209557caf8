"""The crafted ORBmatcher::Fuse cases are what they claim to be, judged by the sequential CPU oracle (tests/cpp/fuse_oracle.cpp): every
named branch of the search and of the tail's three-way switch is reached, every 1-ulp scan holds both outcomes, and the device's
reformulation (search every entry against the map as given, then run the tail in entry order) is shown on a small map model to leave
the very same map as the literal interleaved loop.  The GPU tests (test_gpu_fuse.py) compare the device with this oracle byte for byte
on the same cases.

Contraction: the oracle built with -ffp-contract=fast (and FMA) decides 1,010 of the 3,584 scan points below differently: 246 / 256 of
512 on the mono / stereo chi-square bounds, 256 / 252 on the two strict window bounds, and 0 on the two distance bounds and the
viewing-angle bound, whose deciding quantities (cv::norm, Mat::dot) accumulate in double and whose float products have no addend to
contract with.  test_threshold_scans_see_contraction recounts them and asserts that every float bound has some, so a contracted device
build does not pass the GPU suite unnoticed.

Snapshot semantics: a multi-job call searches every job against the map as given.  test_two_jobs_snapshot pins the one difference from
the sequential reference (a point that a Replace in job 0 made bad is still searched by job 1) and shows that one call per job removes it."""
import numpy as np
import pytest

import fuse_cases as fc
import triangulate_cases as tc

FLOAT_BOUNDS = ("chi2_mono", "chi2_stereo", "window_x", "window_y")


@pytest.fixture(scope="module")
def crafted():
    sc = fc.crafted_scene()
    res, br = fc.cpu_run(sc)
    return sc, res, br


@pytest.fixture(scope="module")
def scans():
    return {k: fc.scan_scene(k) for k in fc.SCAN_KINDS}


def test_crafted_cases_find_what_they_claim(crafted):
    sc, res, _ = crafted
    fc.check_expectations(sc, res)
    names = set(sc["expect"])
    for need in ("d50", "d51", "tie", "closer_out_of_range", "octave_lm1", "octave_l", "octave_lp1", "stereo_fails", "same_offsets_mono",
                 "mono_fails", "uright_zero", "z_negative", "z_zero", "u_eq_maxx", "u_eq_minx", "clip_right", "clip_bottom", "clip_top",
                 "empty_window", "below_min", "above_min", "above_max", "below_max", "angle_61", "angle_59", "skipped", "meet_kf", "meet_bad",
                 "two_on_one_1", "three_on_one_2", "no_features", "out_of_image", "window_66"):
        assert need in names, need


def test_every_named_branch_is_reached(crafted):
    _, _, br = crafted
    missing = [k for k in fc.BRANCHES if br[k] == 0]
    assert not missing, "no crafted case reaches: %s" % missing


def test_tie_goes_to_the_earlier_cell_not_the_lower_index(crafted):
    sc, res, _ = crafted
    job, pos, idx, dist = sc["expect"]["tie"][:4]
    kp = sc["kfs"][0]["kp"]
    other = [i for i in range(len(kp)) if i != idx and abs(float(kp[i]["y"]) - float(kp[idx]["y"])) < 1e-3 and abs(float(kp[i]["x"]) - float(kp[idx]["x"])) < 7]
    assert len(other) == 1 and other[0] < idx, "the loser has the lower index"
    assert fc.cell_of(kp[idx]["x"], kp[idx]["y"])[0] < fc.cell_of(kp[other[0]]["x"], kp[other[0]]["y"])[0]
    assert tuple(res[job][0][pos]) == (idx, dist)


def test_contention_records_who_came_first(crafted):
    sc, res, _ = crafted
    hits = res[0][1]
    for name, n in (("two_on_one", 2), ("three_on_one", 3)):
        pos = [sc["expect"]["%s_%d" % (name, j)][1] for j in range(n)]
        h = [hits[hits["cand"] == p][0] for p in pos]
        assert int(h[0]["action"]) == fc.ADD and int(h[0]["other"]) == -1
        for x in h[1:]:
            assert int(x["action"]) == fc.MEET_CANDIDATE and int(x["other"]) == pos[0] and int(x["idx"]) == int(h[0]["idx"])


def test_empty_job_and_no_features(crafted):
    sc, res, _ = crafted
    assert len(sc["jobs"][3][1]) == 0 and res[3][2] == 0 and len(res[3][0]) == 0 and len(res[3][1]) == 0
    assert len(sc["kfs"][2]["kp"]) == 0 and res[2][2] == 0 and tuple(res[2][0][0]) == (-1, 256)


def test_nfused_counts_every_hit(crafted):
    _, res, _ = crafted
    best, hits, nf = res[0]
    assert nf == len(hits) == int((best[:, 1] <= 50).sum())
    assert set(np.unique(hits["action"])) == {fc.ADD, fc.MEET_KF, fc.MEET_BAD, fc.MEET_CANDIDATE}
    assert np.all(np.diff(hits["cand"]) > 0), "hits come in entry order"


@pytest.mark.parametrize("kind", fc.SCAN_KINDS)
def test_threshold_scans_hold_both_outcomes(scans, kind):
    """512 consecutive-f32 steps in 16 windows across the bound: every window has accepted and rejected items, and acceptance is
    monotonic in the sliding value inside a window (one crossing)."""
    sc = scans[kind]
    ok = fc.scan_accepted(sc)
    assert len(ok) == 512
    per = 512 // fc.SCAN_WINDOWS
    for w in range(fc.SCAN_WINDOWS):
        a = ok[w * per:(w + 1) * per]
        assert a.any() and not a.all(), "%s window %d: one outcome only" % (kind, w)
        assert np.abs(np.diff(a.astype(int))).sum() == 1, "%s window %d: more than one crossing" % (kind, w)


def test_threshold_scans_see_contraction(scans):
    """The same scans through an oracle built with -ffp-contract=fast: the decisions that differ are what the GPU suite would notice of
    a contracted device build.  When written: 3,584 scan points, 1,010 decisions differ; none on the bounds that are decided in double."""
    if not tc.host_has_fma():
        pytest.skip("the host CPU has no FMA: a contracted build cannot run here")
    changed = 0; points = 0
    for kind, sc in scans.items():
        off, fast = fc.scan_accepted(sc), fc.scan_accepted(sc, contract="fast")
        n = int((off != fast).sum())
        print("%s: %d of %d accepted, %d decisions differ under contraction" % (kind, off.sum(), len(off), n))
        if kind in FLOAT_BOUNDS:
            assert n > 0, "%s: no scan decision changes under contraction: densify the scan" % kind
        changed += n; points += len(off)
    print("contraction changes %d of %d scan decisions" % (changed, points))
    assert points == 3584


def test_window_over_64_scene_is_what_it_claims():
    for n in (65, 130):
        sc = fc.dense_window_scene(n)
        res, br = fc.cpu_run(sc)
        assert br["window_over_64"] == len(sc["jobs"][0][1]) and res[0][2] == len(sc["jobs"][0][1])
        assert np.all(res[0][0][:, 1] == 12)


# ---------------------------------------------------------------- the reformulation on the map model
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_search_then_tail_equals_the_literal_fuse(seed):
    """Single jobs: "search every entry on the snapshot, then run the tail in entry order" leaves the model byte-identical to the literal
    interleaved Fuse -- with occupants that win, lose and tie on Observations(), a three-way contention on one feature with
    Observations() 2, 3 and 1, a feature that holds a bad point."""
    sc = fc.model_scene(seed)
    lit, ref = fc.build_model(sc), fc.build_model(sc)
    before = lit.dump()
    assert before == ref.dump()
    n1 = lit.fuse(0, sc["cand"])
    entries, state = ref.snapshot(0, sc["cand"])
    assert np.array_equal(entries, sc["cand"]), "no candidate is in keyframe 0 or bad to begin with"
    assert sorted(np.unique(state).tolist()) == [0, 1, 2]
    best = ref.search(0, sc["cand"])
    n2 = ref.tail(0, sc["cand"], best)
    assert n1 == n2 == int((best[:, 1] <= 50).sum()) and n1 >= 10
    assert lit.dump() == ref.dump() and lit.dump() != before
    _, _, bad, nobs = lit.points()
    for (p, q), (pb, qb) in zip(sc["occupied"], ((1, 0), (0, 1), (0, 1))):     # Observations() 5 > 2: the candidate goes; 2 < 3 and 3 == 3: the occupant
        assert (bad[p], bad[q]) == (pb, qb)
    # the search of the same job through the occupancy-table oracle proposes the same, and names the contention
    (b2, hits, nf), = fc.cpu_run(dict(sc, jobs=[(0, entries, state)]))[0]
    assert b2.tobytes() == best.tobytes() and nf == n1
    con = hits[hits["idx"] == hits[hits["action"] == fc.MEET_CANDIDATE][0]["idx"]]
    assert [int(a) for a in con["action"]] == [fc.ADD, fc.MEET_CANDIDATE, fc.MEET_CANDIDATE] and set(con["other"][1:]) == {int(con["cand"][0])}
    for m in (lit, ref):
        m.close()


def test_two_jobs_snapshot():
    """Fuse(K0, list) then Fuse(K3, list).  Job 0 replaces a candidate by the occupant it meets (Observations() 5 > 2): the candidate is
    bad when the sequential reference reaches job 1 and is skipped there.  A two-job call searched both jobs against the map as given,
    so it still proposes that candidate for K3: the documented difference.  One call per job (snapshot, search, tail; then again) has none."""
    sc = fc.model_scene(0)
    cand = sc["cand"]
    seq = fc.build_model(sc); seq.fuse(0, cand); n_seq = seq.fuse(3, cand)
    multi = fc.build_model(sc)
    e0, _ = multi.snapshot(0, cand); e3, _ = multi.snapshot(3, cand)
    b0, b3 = multi.search(0, cand), multi.search(3, cand)
    multi.tail(0, cand, b0); n_multi = multi.tail(3, cand, b3)
    gone = sc["occupied"][0][0]
    pos = int(np.nonzero(cand == gone)[0][0])
    assert e3[pos] == gone and b3[pos][1] <= 50, "the snapshot still holds the candidate"
    one = fc.build_model(sc)
    one.tail(0, cand, one.search(0, cand))
    e3_late, _ = one.snapshot(3, cand)
    assert e3_late[pos] == -1, "after job 0 the candidate is bad: the reference `continue`s"
    n_one = one.tail(3, cand, one.search(3, cand))
    assert n_multi == n_seq + 1 and multi.dump() != seq.dump()
    assert n_one == n_seq and one.dump() == seq.dump()
    for m in (seq, multi, one):
        m.close()


# ---------------------------------------------------------------- ComputeDistinctiveDescriptors
def _descs(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 7, 33])
def test_distinctive_matches_numpy(n):
    rng = np.random.default_rng(n)
    for _ in range(5):
        d = _descs(rng, n)
        b, out = fc.distinctive(d)
        assert b == fc.distinctive_numpy(d)
        if n == 0:
            assert b == -1 and out is None
        else:
            assert out.tobytes() == d[b].tobytes()


def test_distinctive_small_cases():
    rng = np.random.default_rng(3)
    a = _descs(rng, 1)[0]
    assert fc.distinctive(a[None])[0] == 0
    # N = 2: the median index (int)(0.5 * 1) = 0 is the zero diagonal of both rows: the first wins
    assert fc.distinctive(np.stack([a, fc.flipped(a, 40, rng)]))[0] == 0
    # N = 3: medians are the smaller off-diagonal distance: b (10 from a, 12 from c) has median 10, as has a; a comes first
    b = fc.flipped(a, 10, rng)
    c = tc._flip(b, np.nonzero(np.unpackbits(a ^ b) == 0)[0][:12])         # 12 from b, 22 from a
    assert fc.distinctive(np.stack([a, b, c]))[0] == 0
    assert fc.distinctive(np.stack([c, b, a]))[0] == 1                      # c's median is 12, b's 10: b, the first of the 10s
    # an even N with tied medians: four copies of two descriptors; every median is 0: the first row
    assert fc.distinctive(np.stack([a, b, a, b]))[0] == 0
    # ... and with distinct descriptors in two tight pairs the medians tie pairwise: the first of the best pair
    e = fc.flipped(a, 100, rng); f = fc.flipped(e, 4, rng); g = fc.flipped(a, 6, rng)
    d = np.stack([e, f, a, g])                                                # medians: 4, 4, 6, 6 (sorted row [0, near, far, far], index 1)
    assert fc.distinctive(d)[0] == 0 == fc.distinctive_numpy(d)
    assert fc.distinctive(d[[2, 3, 0, 1]])[0] == 2
