"""The CPU oracle of the device covisibility graph (tests/cpp/covis_oracle.cpp) without a GPU: every crafted case of covis_cases.py reaches
the branches it claims, the literal sequential model (observations stored twice, nObs, SetBadFlag cascades) agrees with the restatement in
the parallel terms of DESIGN.md Q43 (observers derived from the keyframe tables, removals as a set), every deliberately wrong twin is
exposed by a case written for it, and the hand-computed answers the cases are built around hold."""
import numpy as np
import pytest

import covis_cases as cc

CASES = cc.crafted_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_branches_and_matches_the_restatement(case):
    got, br = cc.run_oracle(case["ops"])
    for name in case["claims"]:
        assert br[name] > 0, "%s never reached %s" % (case["name"], name)
    cc.assert_same(got, cc.run_numpy(case["ops"]), case["name"])


def test_every_branch_is_claimed_by_some_case():
    claimed = {b for c in CASES for b in c["claims"]}
    assert claimed == set(cc.BRANCHES), sorted(set(cc.BRANCHES) - claimed)


@pytest.mark.parametrize("twin", [t for t in cc.TWINS if t != "none"])
def test_twin_is_exposed(twin):
    mine = [c for c in CASES if c["twin"] == twin]
    assert mine, "no case written for twin %s" % twin
    for c in mine:
        right, _ = cc.run_oracle(c["ops"])
        wrong, _ = cc.run_oracle(c["ops"], twin=twin)
        assert cc.differs(wrong, right), "%s does not expose %s" % (c["name"], twin)


def _conn(rec):
    return dict(live=rec[1], parent=rec[4], first=rec[5], ordered=list(zip(rec[6], rec[7])), row=dict(zip(rec[8], rec[9])), n_best=rec[10], n_by_weight=rec[11])


def test_known_answers():
    by = {c["name"]: cc.run_oracle(c["ops"])[0] for c in CASES}
    r = by["weights_14_15_16"]
    last = {k: _conn(x) for k, x in zip([0, 1, 2, 3, 4], r[-1])}
    assert last[4]["ordered"] == [(3, 16), (2, 15)] and last[4]["row"] == {1: 14, 2: 15, 3: 16} and last[4]["parent"] == 3 and not last[4]["first"]
    assert last[1]["row"] == {} and last[2]["ordered"] == [(4, 15)] and last[2]["first"] and last[2]["parent"] == -1
    assert (_conn(r[0])["n_best"], _conn(r[0])["n_by_weight"]) == (1, 0)          # weights 16, 15 against 15: upper_bound is the end, the reference returns nothing
    assert (_conn(r[1])["n_best"], _conn(r[1])["n_by_weight"]) == (2, 1) and (_conn(r[2])["n_best"], _conn(r[2])["n_by_weight"]) == (0, 0)
    r = by["none_kept_tied_maxima"][-1]
    assert _conn(r[3])["ordered"] == [(1, 5)] and _conn(r[3])["row"] == {1: 5, 2: 5, 3: 4} and _conn(r[0])["ordered"] == [(5, 5)] and _conn(r[1])["row"] == {}
    r = by["empty_counter_and_bad_points"]
    assert _conn(r[0])["ordered"] == [] and _conn(r[0])["first"] and _conn(r[-1][0])["ordered"] == [(2, 1)]
    r = by["tie_order_descending_id"]
    assert _conn(r[-1][3])["ordered"] == [(3, 20), (2, 20), (1, 20)] and _conn(r[0])["n_by_weight"] == 0 and _conn(r[1])["n_by_weight"] == 0
    r = by["resort_mixes_entries_below_15"]
    assert [_conn(x)["ordered"] for x in r[:4]] == [[(2, 20), (4, 16)], [(2, 20), (4, 16)], [(2, 20), (4, 16)], [(2, 20), (4, 17), (3, 3)]]
    assert _conn(r[4])["n_by_weight"] == 2 and _conn(r[5])["n_by_weight"] == 0
    assert _conn(by["early_return_keeps_the_kept_list"][0])["ordered"] == [(2, 20)]
    r = by["first_connection_and_protected"][-1]
    assert _conn(r[0])["parent"] == -1 and _conn(r[0])["first"] and _conn(r[0])["live"] and _conn(r[1])["parent"] == 0 and _conn(r[1])["ordered"] == [(2, 30), (0, 20)]
    assert _conn(r[2])["parent"] == 1
    r = by["erase_then_update_then_readd"]
    assert _conn(r[0])["ordered"] == [(3, 16)] and _conn(r[0])["row"] == {3: 16}
    assert by["observations_3_4_mono_stereo"][0] == ("cull", [(0, 10, 4), (0, 2, 1), (0, 0, 0), (0, 14, 10)])
    assert by["octave_plus_1_plus_2"][0] == ("cull", [(0, 3, 1)])
    d = by["depth_on_the_threshold"]
    assert d[0] == ("cull", [(1, 5, 5)]) and d[1] == ("cull", [(1, 8, 8)]) and d[2] == ("cull", [(1, 4, 4)])
    for n in (10, 20, 30):
        assert by["bound_0.9_of_%d" % n][0] == ("cull", [(0, n, 9 * n // 10 - 1), (0, n, 9 * n // 10), (1, n, 9 * n // 10 + 1)])
    s = by["first_removal_saves_the_second"]
    assert s[0] == ("cull", [(1, 10, 10), (0, 10, 0)]) and s[1] == ("cull", [(1, 10, 10), (0, 10, 0)])
    s = by["first_removal_saves_the_second_not_erase"]
    assert s[0] == ("cull", [(1, 10, 10), (1, 10, 10)]) and s[1] == ("cull", [(1, 10, 10), (1, 10, 10)])
    s = by["point_driven_bad_by_a_removal"]
    assert s[0] == ("cull", [(1, 11, 10), (1, 9, 9)]) and s[1] == ("cull", [(1, 11, 10), (0, 10, 9)])
    assert by["weighted_observations_after_a_removal"][0] == ("cull", [(1, 11, 10), (0, 10, 9)])
    lm = by["votes_tie_and_bad_entries"][0]
    assert lm[0][1:3] == ([1, 2, 3], 3) and lm[0][5] == [0] * 6 + [1, 0] and lm[0][3] == [0, 1, 2, 3, 4, 5]
    assert lm[1] == ("local", [], -1, [], 0, [1, 0, 0]) and lm[2] == ("local", [], -1, [], 0, []) and lm[3][1:3] == ([1, 3], 1)
    lm = by["neighbour_child_parent_and_the_break"][0]
    assert lm[0][1] == [1, 2, 4, 6] and lm[3][1] == [1, 4, 2, 5, 6]
    for n, size in ((79, 81), (80, 81), (81, 81)):
        r = by["stop_test_with_%d_voted" % n][0][0]
        assert len(r[1]) == size and r[4] == n
    r = by["a_dead_neighbour_is_skipped"]
    assert _conn(r[0])["ordered"] == [(2, 16), (3, 15)] and not _conn(r[-1][1])["live"] and r[1][0][1] == [1, 3, 2]       # the parent is appended without an isBad() test, as in the reference


@pytest.mark.parametrize("seed", range(2))
def test_random_scripts_match_the_restatement(seed):
    ops = cc.random_script(seed)
    got, br = cc.run_oracle(ops)
    cc.assert_same(got, cc.run_numpy(ops), "random %d" % seed)
    assert br["ac_changed"] > 0 and br["er_connection"] > 0 and br["cu_flagged"] > 0 and br["lm_parent_break"] > 0 and br["uc_w16"] > 0
