"""The CPU oracle of the device KeyFrameDatabase (tests/cpp/kfdb_oracle.cpp) without a GPU: every crafted case of kfdb_cases.py reaches the
branch it claims, the literal sequential algorithm agrees byte for byte with the numpy restatement in the parallel terms of DESIGN.md
Q42, every deliberately wrong twin is exposed by a case written for it, and the score is the project's orc_bow_score_l1."""
import numpy as np
import pytest

import kfdb_cases as kc

CASES = kc.crafted_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_branches_and_matches_the_restatement(case):
    got, br = kc.run_oracle(case["ops"], case["max_kf"])
    for name in case["claims"]:
        assert br[name] > 0, "%s never reached %s" % (case["name"], name)
    kc.assert_same(got, kc.run_numpy(case["ops"], case["max_kf"]), case["name"])


def test_every_branch_is_claimed_by_some_case():
    claimed = {b for c in CASES for b in c["claims"]}
    assert claimed == set(kc.BRANCHES), sorted(set(kc.BRANCHES) - claimed)


@pytest.mark.parametrize("twin", [t for t in kc.TWINS if t != "none"])
def test_twin_is_exposed(twin):
    mine = [c for c in CASES if c["twin"] == twin]
    assert mine, "no case written for twin %s" % twin
    for c in mine:
        right, _ = kc.run_oracle(c["ops"], c["max_kf"])
        wrong, _ = kc.run_oracle(c["ops"], c["max_kf"], twin=twin)
        assert kc.differs(wrong, right), "%s does not expose %s" % (c["name"], twin)


def test_known_answers():
    """The hand-computed outcomes the cases are built around."""
    by = {c["name"]: kc.run_oracle(c["ops"], c["max_kf"])[0] for c in CASES}
    r = by["min_score"][0]
    assert list(r[0]["candidates"]) == [0, 2] and r[0]["info"]["nscores"] == 3 and list(r[1]["candidates"]) == []
    for form in ("loop", "reloc"):
        r = by["retain_" + form][0][0]
        assert list(r["candidates"]) == [0, 2] and r["info"]["min_score_to_retain"] == np.float32(0.75) and r["info"]["n_acc"] == 4
        r = by["neighbour_scores_" + form][0][0]
        assert r["acc"][0]["best_kf"] == 2 and r["acc"][0]["acc_score"] == np.float32(2.5)
    for m, minc in ((1, 0), (4, 3), (5, 4), (10, 8), (15, 12)):
        r = by["min_common_%d_loop" % m][0][0]
        assert r["info"]["min_common_words"] == minc and r["info"]["nscores"] == len({m, minc + 1})
    z = by["zero_weight"]
    assert z[0][0]["sharing"]["si"].tobytes() == np.float32(-0.0).tobytes() and len(z[0][0]["candidates"]) == 0
    assert z[0][0]["info"]["best_acc_score"].tobytes() == np.float32(0.0).tobytes() and z[1][0]["info"]["n_acc"] == 1 and list(z[1][0]["candidates"]) == []
    assert z[2][0].tobytes() == np.array([-0.0, -1.0], np.float32).tobytes()
    s = by["sum_order"]
    assert s[0][0]["sharing"]["si"][0] == np.float32(1.0) and s[2][0][0] == np.float32(1.0)
    lo = by["list_order"]
    assert list(lo[0][0]["sharing"]["kf_id"]) == [6, 5, 2, 7, 1, 3] and list(lo[2][0]["sharing"]["kf_id"]) == [6, 2, 7, 5, 1, 3]
    ex = by["excluded"][0]
    assert 1 not in ex[0]["sharing"]["kf_id"] and list(ex[0]["candidates"]) == [0] and ex[0]["acc"][0]["acc_score"] == np.float32(1.0) and list(ex[1]["candidates"]) == [1]
    d = by["dup_best"]
    assert list(d[0][0]["candidates"]) == [1, 3] and list(d[0][0]["acc"]["best_kf"]) == [1, 3, 1, 1]
    two = by["reloc_two_calls"]
    assert list(two[0][0]["candidates"]) == [2] and list(two[2][0]["candidates"]) == [0, 2] and two[2][0]["acc"][0]["acc_score"] == np.float32(1.0)
    one = by["reloc_one_call"]
    assert list(one[0][1]["candidates"]) == [0, 2] and list(one[1][0]["candidates"]) == [2]
    assert list(by["reloc_readd"][1][0]["candidates"]) == [2] and list(by["reloc_readd"][2][1]["candidates"]) == [0, 2]
    assert list(by["loop_gate"][1][0]["candidates"]) == [2]


def test_score_is_the_projects_l1(orc):
    rng = np.random.default_rng(3)
    for _ in range(20):
        a = kc.random_bow(rng, int(rng.integers(1, 80)), 200); b = kc.random_bow(rng, int(rng.integers(1, 80)), 200)
        want = orc.bow_score_l1(dict(word=a[0], value=a[1]), dict(word=b[0], value=b[1]))
        assert kc.l1(a, b) == want
    v = ([1, 2, 3], [0.5, 0.25, 0.25])
    assert kc.l1(v, v) == 1.0


@pytest.mark.parametrize("seed", range(2))
def test_random_scripts_match_the_restatement(seed):
    ops = kc.random_script(seed, n_entries=90, max_kf=128, vocab=150, words=(1, 25), n_calls=6, queries_per_call=3)
    got, br = kc.run_oracle(ops, 128)
    kc.assert_same(got, kc.run_numpy(ops, 128), "random %d" % seed)
    assert br["neigh_better"] > 0 and br["excluded_hit"] > 0 and br["neigh_unscored_reloc"] > 0 and br["several_common"] > 0
