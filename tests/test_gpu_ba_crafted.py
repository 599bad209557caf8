"""Optimizer::LocalBundleAdjustment on the GPU (k_ba.h through frontend.local_bundle_adjustment) on the crafted cases of ba_crafted.py.
EXACT cases: byte for byte against the outcome known by construction (poses and points keep the input's bytes, the flags written down
by hand, the counts of the rho == 0 ending).  Cached-error cases: the numpy recomputation on the device's own output.  Orders, list
lengths and sizes: decisions and counts equal to the oracle fed the same order, values within max(10 x the case's recorded spread
(profiles/ba_crafted_tolerance.json), 4 f32 ulps of the entry): DESIGN Q37.  test_ba_crafted.py shows on the CPU that agreeing with the
oracle on these cases rules out each of the oracle's wrong twins."""
import json
import os

import numpy as np
import pytest

import ba_cases as bc
import ba_crafted as cr

pytestmark = pytest.mark.gpu
EXACT = list(cr.EXACT)
SEEDED = list(cr.SEARCHED) + list(cr.SCENES)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(bc.ROOT, "profiles", "ba_crafted_tolerance.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def exact_out(gpu, fe):
    """Every exact problem in one launch."""
    return dict(zip(EXACT, fe.local_bundle_adjustment([bc.problem_of(cr.exact_case(n)["scene"]) for n in EXACT])))


@pytest.fixture(scope="module")
def seeded_out(gpu, fe):
    """Every seeded problem in one launch; the cap case sizes the launch's LDS request."""
    return dict(zip(SEEDED, fe.local_bundle_adjustment([bc.problem_of(cr.scene(n)) for n in SEEDED])))


def same_bits(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in ("Tcw", "xw", "normal", "dist", "level1", "erase", "stats"))


def agrees(name, got, want, spread):
    bad = bc.mismatch(got, want, spread, log=lambda t: print(name, t))
    assert bad is None, "%s: %s" % (name, bad)
    for rnd in (0, 1):                                     # as test_gpu_ba.py; an infinite chi2 (last_trial_rejected) has to be infinite
        g, w = got["stats"]["chi2"][rnd], want["stats"]["chi2"][rnd]
        assert g == w or abs(g - w) <= 1e-9 * max(w, 1.0), (name, rnd, g, w)


@pytest.mark.parametrize("name", EXACT)
def test_exact_case_byte_for_byte(exact_out, recorded, name):
    got = exact_out[name]
    cr.assert_by_construction(name, got)
    # device and oracle agree exactly: nothing moved, so also the normals and distances have one value
    assert recorded[name] == {kind: 0.0 for kind, _ in bc.KINDS}
    # (the chi2 the construction states -- 0, infinite, a sum of f32 values -- is held exactly above; round 1 of probe_thresholds is a
    # sum of Huber terms 2 sqrt(chi2) delta - delta^2, which are not f32 values: its last bit follows the order of the sum)
    agrees(name, got, cr.expected(name), recorded[name])


def test_last_trial_rejected_reads_the_rejected_trials_error(exact_out):
    c, got = cr.exact_case("last_trial_rejected"), exact_out["last_trial_rejected"]
    prob = bc.problem_of(c["scene"])
    assert got["stats"]["rejected"].tolist() == got["stats"]["trials"].tolist() == [5, 1]
    fresh = cr.fresh_chi2(prob, got["Tcw"], got["xw"])     # the restored estimates are the returned ones
    assert (fresh[c["pair"]] > cr.bounds_of(prob)[c["pair"]]).all() and (got["level1"][c["pair"]] == 0).all()
    assert (got["erase"][c["pair"]] == 1).all()


@pytest.mark.parametrize("name", SEEDED)
def test_seeded_case_matches_oracle(seeded_out, recorded, name):
    agrees(name, seeded_out[name], cr.expected(name), recorded[name])


def test_stale_level1_is_erased_on_its_cached_error(seeded_out):
    prob, got = bc.problem_of(cr.scene("stale_level1")), seeded_out["stale_level1"]
    idx = cr.stale_level1_edges(prob, got)                 # level 1, point still active, erased, fresh chi2 below half the bound
    assert np.array_equal(idx, cr.stale_level1_edges(prob, cr.expected("stale_level1"))) and len(idx) >= 1


def test_fixed_byte_on_fixed_cameras_changes_nothing(seeded_out):
    assert same_bits(seeded_out["fixed_byte_0"], seeded_out["fixed_byte_1"])


def test_caps_as_second_problem_after_a_small_one(fe, seeded_out):
    """The LDS is sized from the largest problem of the launch: the cap case behind `small`, and each of them, answer as they do in
    any other launch."""
    small, caps = fe.local_bundle_adjustment([bc.problem_of(bc.scene("small")), bc.problem_of(cr.scene("size_caps"))])
    assert same_bits(caps, seeded_out["size_caps"])
    assert same_bits(small, fe.local_bundle_adjustment([bc.problem_of(bc.scene("small"))])[0])
