"""The crafted LocalBundleAdjustment cases of ba_crafted.py on the CPU: the constructions are exact, the oracle (tests/cpp/ba_oracle.cpp)
meets every outcome that is known by construction, each deliberately wrong twin of the oracle differs from it on the case named for
it, the cached-error cases show their stale / fresh split by a numpy recomputation, and every seeded case keeps the margin and has its
spread recorded (profiles/ba_crafted_tolerance.json, the yardstick of test_gpu_ba_crafted.py; DESIGN Q37)."""
import json
import os

import numpy as np
import pytest

import ba_cases as bc
import ba_crafted as cr

TOLERANCE_JSON = os.path.join(bc.ROOT, "profiles", "ba_crafted_tolerance.json")
ZERO = {kind: 0.0 for kind, _ in bc.KINDS}
SEEDED = list(cr.SEARCHED) + list(cr.SCENES)


@pytest.mark.parametrize("name", list(cr.EXACT))
def test_oracle_meets_the_outcome_known_by_construction(name):
    r = cr.expected(name)
    cr.assert_by_construction(name, r)
    # one Quaterniond(Matrix3d) branch per orientation, a local and a fixed keyframe each
    for b in cr.QUAT_BRANCH.values():
        assert r["branches"][b] >= 2, (name, b, r["branches"])
    assert r["branches"]["factor_fail"] == 0


def test_exact_scenes_use_every_orientation_kind_and_side():
    for kind, mono, stereo in (("mono", True, False), ("stereo", False, True), ("mixed", True, True)):
        e = cr.exact_case("exact_" + kind)["scene"]["edges"]
        assert (e["ur"] < 0).any() == mono and (e["ur"] >= 0).any() == stereo
        assert set(e["kf"].tolist()) == set(range(8))
    r = cr.expected("probe_thresholds")
    assert r["branches"]["level1_chi2"] == 16 and r["branches"]["level1_depth"] == 0 and r["margins"]["chi2"] < 1e-7
    r, c = cr.expected("probe_depth"), cr.exact_case("probe_depth")
    assert r["branches"]["level1_depth"] == 9 and r["branches"]["level1_chi2"] == 0
    e = c["scene"]["edges"][c["level1"] == 1]
    assert (e["kf"] < 4).any() and (e["kf"] >= 4).any() and (e["ur"] < 0).any() and (e["ur"] >= 0).any()
    assert (r["cached"][:, c["level1"] == 1] == 0).all()                      # flagged by depth alone: their chi2 is exactly 0


def differs(name, twin, scene, base, spread):
    got = bc.run_oracle(bc.problem_of(scene), twin=twin)
    bad = bc.mismatch(got, base, spread)
    assert bad is not None, "the twin %s passes for the oracle on %s" % (twin, name)
    return bad


def test_twin_f32_compare_differs_on_probe_thresholds():
    bad = differs("probe_thresholds", "f32_compare", cr.exact_case("probe_thresholds")["scene"], cr.expected("probe_thresholds"), ZERO)
    assert "n_level1" in bad


def test_twin_no_depth_test_differs_on_probe_depth():
    bad = differs("probe_depth", "no_depth_test", cr.exact_case("probe_depth")["scene"], cr.expected("probe_depth"), ZERO)
    assert "n_level1" in bad


def test_twin_fresh_chi2_differs_on_both_cached_error_cases():
    differs("stale_level1", "fresh_chi2", cr.scene("stale_level1"), cr.expected("stale_level1"), spread("stale_level1"))
    bad = differs("last_trial_rejected", "fresh_chi2", cr.exact_case("last_trial_rejected")["scene"], cr.expected("last_trial_rejected"), ZERO)
    assert "n_level1" in bad


def test_twins_of_the_two_rounds_differ_on_their_cases():
    with open(os.path.join(bc.ROOT, "profiles", "ba_tolerance.json")) as f:
        recorded = json.load(f)["cases"]
    differs("outliers", "level1_active", bc.scene("outliers"), bc.expected("outliers"), recorded["outliers"])
    assert bc.expected("mixed")["Tcw"].tobytes() != bc.scene("mixed")["kfs"]["Tcw"][:3].tobytes()      # a case that moves
    differs("mixed", "lambda_carried", bc.scene("mixed"), bc.expected("mixed"), recorded["mixed"])
    assert cr.expected("stereo_between")["branches"]["stereo_between"] > 0
    differs("stereo_between", "delta_swapped", cr.scene("stereo_between"), cr.expected("stereo_between"), spread("stereo_between"))


def test_flags_zero_is_the_oracle_and_no_twin_is():
    assert sorted(bc.TWINS.values()) == [1, 2, 4, 8, 16, 32]
    s, r = bc.scene("mixed"), bc.expected("mixed")
    again = bc.run_oracle(bc.problem_of(s), twin=None)
    assert all(again[k].tobytes() == r[k].tobytes() for k in ("Tcw", "xw", "normal", "dist", "level1", "erase", "stats"))


def test_stale_level1_is_erased_on_its_cached_error():
    s, r = cr.scene("stale_level1"), cr.expected("stale_level1")
    prob = bc.problem_of(s)
    idx = cr.stale_level1_edges(prob, r)
    assert len(idx) >= 1 and r["branches"]["level1_point_active"] >= len(idx)
    fresh, bound = cr.fresh_chi2(prob, r["Tcw"], r["xw"]), cr.bounds_of(prob)
    print("stale_level1 (seed %d): edges %s fresh chi2 %s cached %s bound %s" % (s["seed"], idx, fresh[idx], r["cached"][1][idx], bound[idx]))
    assert (fresh[idx] < 0.5 * bound[idx]).all() and (r["erase"][idx] == 1).all()
    # the value the erase test read is the one round 1 left, and it is above the bound
    assert np.array_equal(r["cached"][1][idx], r["cached"][0][idx]) and (r["cached"][1][idx] > bound[idx]).all()
    # the numpy recomputation is the oracle's arithmetic where both are fresh: the level-0 edges after an accepted last trial
    assert r["branches"]["last_rejected_r2"] == 0
    live = r["level1"] == 0
    assert np.allclose(fresh[live], r["cached"][1][live], rtol=1e-3, atol=1e-6)


def test_last_trial_rejected_is_classified_on_the_rejected_trials_error():
    c, r = cr.exact_case("last_trial_rejected"), cr.expected("last_trial_rejected")
    prob = bc.problem_of(c["scene"])
    assert r["branches"]["last_rejected_r1"] == 1 and r["branches"]["last_rejected_r2"] == 1
    # round 1 restored the input, so the fresh chi2 at classification is the input's: 64 on the pair, far above the bound ...
    fresh = cr.fresh_chi2(prob, r["Tcw"], r["xw"])
    assert (fresh[c["pair"]] == 64.0).all() and (fresh[c["pair"]] > cr.bounds_of(prob)[c["pair"]]).all()
    # ... while the cached one is the rejected trial's NaN: the other side of the bound (NaN > bound is false)
    assert np.isnan(r["cached"][0][c["pair"]]).all() and (r["level1"][c["pair"]] == 0).all()
    assert (r["cached"][1][c["pair"]] == 64.0).all() and (r["erase"][c["pair"]] == 1).all()


def test_no_finite_seed_has_a_rejected_last_trial_with_a_split():
    """Why last_trial_rejected is built and not searched: over 200 far starts every round that ends on a rejected trial ends on the tenth
    rejection in a row, where cached and fresh chi2 agree and rho is rounding noise inside the margin."""
    hits = 0
    for seed in range(800, 1000):
        s = bc.make_scene(seed, 3, 2, 30, stereo_frac=0.5, noise=1.0, pose_noise=(0.1, 0.5), point_noise=0.8, mild=0.05)
        prob = bc.problem_of(s)
        r = bc.run_oracle(prob)
        if not r["branches"]["last_rejected_r2"]:
            continue
        hits += 1
        assert r["stats"]["rejected"][1] >= 10 and r["margins"]["rho"] < bc.MARGIN
        live = r["level1"] == 0
        fresh = cr.fresh_chi2(prob, r["Tcw"], r["xw"])
        assert np.allclose(fresh[live], r["cached"][1][live], rtol=1e-3, atol=1e-6)
    assert hits >= 1


# ---------------------------------------------------------------- seeded cases: conditions, structure, yardstick
_spreads = {}


def spread(name):
    if name not in _spreads:
        s = cr.exact_case(name)["scene"] if name in cr.EXACT else cr.scene(name)
        sp = bc.spread_of(bc.problem_of(s), cr.expected(name))
        assert sp is not None, "%s: a variant of the oracle takes another decision" % name
        _spreads[name] = sp
    return _spreads[name]


@pytest.mark.parametrize("name", SEEDED)
def test_every_decision_is_outside_the_margin(name):
    r = cr.expected(name)
    for k, v in r["margins"].items():
        assert v >= bc.MARGIN, "%s: a %s decision at relative distance %.3g from its threshold" % (name, k, v)
    assert r["branches"]["factor_fail"] == 0


def test_searched_cases_are_the_first_seed_of_their_search():
    for name, (build, want, seeds) in cr.SEARCHED.items():
        assert cr.scene(name)["seed"] in seeds


def per_kf(s):
    return np.bincount(s["edges"]["kf"], minlength=len(s["kfs"]))


def test_insertion_orders_hold_the_same_edges():
    base = cr.scene("order_point_major")
    e = base["edges"]
    assert base["n_local"] >= 3 and len(base["kfs"]) - base["n_local"] >= 2 and len(e) == 300
    assert (np.diff(e["point"]) >= 0).all()
    key = lambda a: sorted(a.tolist())
    for o in cr.ORDERS[1:]:
        f = cr.scene("order_" + o)["edges"]
        assert key(f["tag"]) == key(e["tag"]) and not np.array_equal(f["tag"], e["tag"])
        assert np.array_equal(np.sort(f, order="tag"), np.sort(e, order="tag"))
    assert (np.diff(cr.scene("order_kf_major")["edges"]["kf"]) >= 0).all()
    assert np.array_equal(cr.scene("order_reversed")["edges"], e[::-1])
    # every order takes the same decisions, and its own oracle run is what the device is held to
    want = cr.expected("order_point_major")
    for o in cr.ORDERS[1:]:
        r = cr.expected("order_" + o)
        by_tag = np.argsort(cr.scene("order_" + o)["edges"]["tag"], kind="stable")
        assert np.array_equal(r["erase"][by_tag], want["erase"][np.argsort(e["tag"], kind="stable")])
        assert all(np.array_equal(r["stats"][f], want["stats"][f]) for f in bc.COUNTS)


def test_same_key_chunks_and_list_lengths():
    for n in (256, 257):
        e = cr.scene("chunk_%d" % n)["edges"]
        assert (per_kf(cr.scene("chunk_%d" % n)) == n).all() and (np.diff(e["kf"]) >= 0).all()
        chunks = [e["kf"][c:c + bc.THREADS] for c in range(0, len(e), bc.THREADS)]
        one_key = [len(set(c.tolist())) == 1 for c in chunks]
        # 257: every later full chunk begins inside one keyframe's list and ends inside the next one's
        assert all(one_key) if n == 256 else (one_key[0] and not any(one_key[1:-1]) and len(chunks[-1]) < bc.THREADS)
    s = cr.scene("list_lengths")
    assert tuple(per_kf(s)[:4].tolist()) == cr.LIST_LENGTHS == (63, 64, 65, 129) and s["n_local"] == 4
    assert (np.diff(s["edges"]["kf"]) >= 0).all()


def test_reduced_system_sizes_and_the_caps():
    for name, n_local, n_fixed in (("size_16", 16, 3), ("size_63", 63, 3), ("size_caps", cr.MAX_LOCAL, cr.MAX_FIXED)):
        s, r = cr.scene(name), cr.expected(name)
        assert s["n_local"] == n_local and len(s["kfs"]) == n_local + n_fixed
        assert per_kf(s)[:n_local].min() >= 12, (name, per_kf(s)[:n_local].min())       # an under-determined pose would test nothing
        assert (s["edges"]["point"] == 0).sum() == n_local + n_fixed                     # one point seen by every keyframe
        assert r["branches"]["pose_pose"] > 0 and r["stats"]["iterations"].min() >= 2
        assert np.abs(r["Tcw"].reshape(-1, 16) - s["kfs"]["Tcw"][:n_local]).max() > 1e-3 # it moves
    assert 6 * 16 == 2 * bc.CHOL_TILE and 6 * cr.MAX_LOCAL == 8 * bc.CHOL_TILE
    assert (cr.scene("size_caps")["edges"]["point"] == 0).sum() >= 192


def test_block_sparse_groups_share_no_point():
    s = cr.scene("block_sparse")
    e = s["edges"]
    pts = lambda ks: set(e["point"][np.isin(e["kf"], ks)].tolist())
    a, b, c = pts([0, 1, 2]), pts([3, 4, 5]), pts([6])
    assert a and b and c and not (a & b) and not (a & c) and not (b & c)
    assert c <= pts([7, 8]) and per_kf(s)[:7].min() >= 12                               # keyframe 6's points: fixed cameras only besides it


def test_fixed_byte_on_fixed_cameras_changes_nothing():
    a, b = cr.scene("fixed_byte_0"), cr.scene("fixed_byte_1")
    assert (a["kfs"]["fixed"][a["n_local"]:] == 0).all() and (b["kfs"]["fixed"][b["n_local"]:] == 1).all()
    assert np.array_equal(a["edges"], b["edges"]) and a["xw"].tobytes() == b["xw"].tobytes()
    ra, rb = cr.expected("fixed_byte_0"), cr.expected("fixed_byte_1")
    assert all(ra[k].tobytes() == rb[k].tobytes() for k in ("Tcw", "xw", "normal", "dist", "level1", "erase", "stats"))


def test_tolerance_yardstick_is_recorded():
    rec = {name: spread(name) for name in list(cr.EXACT) + SEEDED}
    for name, sp in rec.items():
        assert max(sp.values()) < 2e-5, (name, sp)
    text = json.dumps(dict(what="largest |difference| of the oracle's f32 outputs between the build with -ffp-contract=off and (a) "
                                "-ffp-contract=fast, (b) the edges in reversed insertion order; per crafted case of tests/ba_crafted.py",
                           cases=rec), indent=1, sort_keys=True) + "\n"
    old = open(TOLERANCE_JSON).read() if os.path.exists(TOLERANCE_JSON) else None
    if old != text:
        with open(TOLERANCE_JSON, "w") as f:
            f.write(text)
