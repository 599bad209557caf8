"""CPU side of bow_cases.py: the crafted trees, descriptors and pairs hold what their names claim (every distance, tie, depth, count
and straddle is recomputed from the bits); the oracle agrees with the numpy restatements on every case, f64 values as uint64; every
mutant of the restatements differs from the oracle on a case built for it; and, where oracle/_ref/libdbow2_ref.so was built, the
BowVector / FeatureVector of the `weights` and `sizes` cases equal those of the reference's own classes."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import bow_cases as bc
import triangulate_cases as tc

REF_SO = os.path.join(graft.ROOT, "oracle", "_ref", "libdbow2_ref.so")
ALL = ("word", "value", "fv_node", "fv_feature", "f_word", "f_weight", "f_node")
COMBOS = [(s, w) for s in range(6) for w in range(4)]


@pytest.fixture(scope="module")
def ties(orc):
    g = bc.ties(); g["O"] = orc.Vocabulary.from_nodes(g["voc"])
    return g


@pytest.fixture(scope="module")
def depths(orc):
    g = bc.depths(); g["O"] = orc.Vocabulary.from_nodes(g["voc"])
    return g


@pytest.fixture(scope="module")
def weights():
    return bc.weights()


@pytest.fixture(scope="module")
def sizes():
    return bc.sizes()


@pytest.fixture(scope="module")
def pairs(synth, orc):
    voc = tc.vocabulary(synth, 5)
    O = orc.Vocabulary.from_nodes(voc)
    voc, groups = bc.kf_frame_cases(synth, orc, O)
    groups["random"] = [bc.random_case(voc, O, s, r, m) for s, r, m in ((0, 0.7, True), (1, 0.75, True), (2, 0.75, False))]
    return voc, O, groups


# ---------------------------------------------------------------- the inputs hold what they claim
def test_tie_probes(ties):
    ch, nd, _, nword = bc.children_of(ties["voc"])
    assert ties["voc"]["k"] == 20 and max(len(c) for c in ch) == 20
    assert np.array_equal(nd[ch[0][3]], nd[ch[0][17]]) and np.array_equal(nd[ch[8][3]], nd[ch[8][17]])
    word, _, _ = bc.numpy_transform(ties["voc"], ties["desc"], 0)
    seen = set()
    for i, (name, (parent, level, tied, dist)) in enumerate(zip(ties["names"], ties["claims"])):
        d = bc.dists(ties["desc"][i], nd[ch[parent]])
        assert d.min() == dist and np.nonzero(d == d.min())[0].tolist() == tied, "%s: distances %r" % (name, d)
        if level == 2:                                       # the probe reaches that parent: it is the nearest level-1 child, alone
            d1 = bc.dists(ties["desc"][i], nd[ch[0]])
            assert ch[0][int(np.argmin(d1))] == parent and (d1 == d1.min()).sum() == 1, name
            assert ch[0].index(parent) > 0, "the level-2 ties sit under a child that is not the first"
        assert word[i] == nword[ch[parent][tied[0]]], "%s: the first of the tied children is a word and the probe lands on it" % name
        seen.add((level, len(tied) > 1, any(t >= 16 for t in tied) and any(t < 16 for t in tied)))
    assert {(1, True, True), (2, True, True), (1, True, False), (2, True, False)} <= seen, "ties inside a round and across the rounds, at both levels"
    assert 256 in [int(bc.dists(ties["desc"][i], nd[ch[c[0]]]).max()) for i, c in enumerate(ties["claims"])], "a distance of 256 occurs"


def test_depth_features(depths):
    voc = depths["voc"]
    ch, nd, _, nword = bc.children_of(voc)
    assert len(ch[depths["single_child"]]) == 1 and voc["L"] == 5 and voc["k"] == 3
    levels = [c[1] for c in depths["claims"]]
    assert levels[:8] == [1, 2, 3, 5, 1, 2, 3, 5] and len(levels) == 64, "four consecutive features, four depths"
    kinds = set()
    for levelsup in range(0, voc["L"] + 2):
        word, _, nid = bc.numpy_transform(voc, depths["desc"], levelsup)
        nid_level = voc["L"] - levelsup
        for i, (leaf, lvl) in enumerate(depths["claims"]):
            assert word[i] == nword[leaf], "%s ends on another leaf" % depths["names"][i]
            if nid_level <= 0:
                assert nid[i] == 0; kinds.add("root")
            elif lvl < nid_level:
                assert nid[i] == leaf; kinds.add("unset_in_the_reference")
            elif lvl == nid_level:
                assert nid[i] == leaf; kinds.add("leaf")
            else:
                assert nid[i] != leaf and len(ch[nid[i]]) > 0; kinds.add("interior")
    assert kinds == {"root", "unset_in_the_reference", "leaf", "interior"}


def test_weights_and_sizes(weights, sizes):
    voc = weights["voc"]
    w = voc["weight"][voc["is_leaf"] > 0]
    assert len(w) == 100 and voc["k"] == 10 and voc["L"] == 2 and [i for i in range(100) if w[i] == 0] == list(bc.ZERO_WORDS)
    nz = w[w > 0]
    assert np.log10(nz.max() / nz.min()) > 10.5, "the weights span about 12 decades"
    assert np.mean((nz.view(np.uint64) & 0xFFFF) != 0) > 0.95, "full mantissas"
    word, wt, nid = bc.numpy_transform(voc, weights["desc"], 1)
    assert word.tolist() == weights["claims"], "every feature lands on its word"
    counts = np.bincount(word, minlength=100)
    assert all(counts[wd] == c for wd, c in bc.HITS.items()) and sorted(set(bc.HITS.values())) == [1, 2, 3, 5, 7, 70]
    first = {wd: int(np.nonzero(word == wd)[0][0]) for wd in bc.HITS}
    last = {wd: int(np.nonzero(word == wd)[0][-1]) for wd in bc.HITS}
    assert first[69] < last[47] and first[47] < last[69], "the repeated words interleave in feature order"
    for name, d in sizes["frames"].items():
        word, wt, nid = bc.numpy_transform(sizes["voc"], d, 1)
        assert word.tolist() == sizes["words"][name].tolist(), name
    assert sorted(bc.sort_size(n)[0] for n in bc.SIZES) == [256] * 7 + [512] * 2 + [1024] * 2 + [2048]
    for n in (513, 1025):
        word, wt, nid = bc.numpy_transform(sizes["voc"], sizes["frames"]["n%d" % n], 1)
        run, rep, per = bc.straddles(word, wt, nid)
        assert run and rep and per == {513: 4, 1025: 8}[n], "N = %d: a run and a repeated word lie across a chunk boundary" % n
    for nb in (64, 65):
        v = bc.numpy_bow(sizes["voc"], sizes["frames"]["nb%d" % nb], 1)
        assert len(v["word"]) == nb and len(v["fv_feature"]) == nb + 9
    v = bc.numpy_bow(sizes["voc"], sizes["frames"]["one_word"], 1)
    assert v["word"].tolist() == [69] and len(v["fv_feature"]) == 40 and v["value"].tolist() == [1.0]


def test_pair_cases(pairs, orc):
    voc, O, g = pairs
    for c in [x for grp in g.values() for x in grp]:
        if c["want"]:
            tc.check_distances(c["kf"], c["frame"], c["want"])
    outcomes = set()
    for c in g["edges"][:2]:
        m, _ = bc.oracle_kf_frame(orc, c)
        a, b = c["notes"]["d50"]; assert m[b] == a
        a, b = c["notes"]["d51"]; assert m[b] == -1
        a, b = c["notes"]["single"]; assert m[b] == a and (c["frame"]["fv"][0] == c["frame"]["fv"][0][list(c["frame"]["fv"][1]).index(b)]).sum() == 1
        a, b = c["notes"]["masked"]; assert m[b] == -1 and c["valid"][a] == 0
        r = np.float32(c["nnratio"])
        for a, b, d1, d2 in c["notes"]["ratio"]:
            assert (m[b] == a) == bool(np.float32(d1) < r * np.float32(d2)), "the oracle applies the rule as written (%d, %d, %g)" % (d1, d2, c["nnratio"])
            outcomes.add((c["nnratio"], bool(m[b] == a), d1 == int(np.floor(float(r) * d2))))
        nk, nf = set(c["kf"]["fv"][0].tolist()), set(c["frame"]["fv"][0].tolist())
        assert min(nk) < min(nf) and max(nk) > max(nf) and nf - nk and nk - nf, "nodes of one side only, at both ends of the frame's list"
    for r in (0.7, 0.75):
        assert {(r, True, False), (r, False, False)} <= outcomes and any(o[0] == r and o[2] for o in outcomes), "both sides of the ratio edge at %g" % r
    for c in g["edges"][2:]:
        assert len(set(c["kf"]["fv"][0].tolist()) & set(c["frame"]["fv"][0].tolist())) == 20 > 16
    assert g["edges"][3]["valid"] is None
    c = g["contention"][0]
    node, feat = c["kf"]["fv"]
    a, b = c["notes"]["pos63"]
    run = feat[node == node[list(feat).index(a)]]
    assert len(run) == 70 and list(run).index(a) == 63 and list(run).index(b) == 64
    node, feat = c["frame"]["fv"]
    f, h = c["notes"]["second_slot"]
    run = feat[node == node[list(feat).index(f)]]
    assert bc.REGF >= len(run) > 64 and list(run).index(f) >= 64 and list(run).index(h) >= 64
    m, _ = bc.oracle_kf_frame(orc, c); bc.check_expect(c, m)
    for c, n in zip(g["node_sizes"], (64, 65, 128, 129)):
        assert np.bincount(c["frame"]["fv"][0]).max() == n
        m, nm = bc.oracle_kf_frame(orc, c)
        close = np.arange(n - 12, n)
        assert nm >= 12 and (m[close] >= 0).sum() >= 10, "the close candidates at the end of the list are found"
    assert len(set(g["node_sizes"][3]["frame"]["fv"][0].tolist())) == 4, "small nodes next to the 129-feature node"
    for c in g["rotation"] + g["tie"] + g["masks"] + g["empty"] + g["edges"][2:]:
        m, _ = bc.oracle_kf_frame(orc, c); bc.check_expect(c, m)
    rot = g["rotation"][0]
    ang = rot["kf"]["kp"]["angle"][:, None] - rot["frame"]["kp"]["angle"][None, :]
    assert (np.diag(ang) < 0).any() and (np.diag(ang) >= 885).any(), "rot < 0 and bin == 30 occur"
    m, nm = bc.oracle_kf_frame(orc, rot); assert nm == 36, "three equal maxima of 12 keep their matches"
    sc = g["scan"][0]
    m, _ = bc.oracle_kf_frame(orc, sc)
    kept = m[sc["notes"]["first_probe"]:] >= 0
    assert (~kept[:8]).all() and kept[8:].all() and (m[:sc["notes"]["first_probe"]] >= 0).all(), "the scan flips once, in its middle"
    for c in g["empty"]:
        assert bc.oracle_kf_frame(orc, c)[1] == 0
    assert [len(c["kf"]["kp"]) for c in g["empty"]] == [0, 1, 1, 1] and [len(c["frame"]["kp"]) for c in g["empty"]] == [1, 0, 1, 1]
    assert g["masks"][0]["kf"] is g["masks"][1]["kf"]
    for c in g["random"]:
        assert bc.oracle_kf_frame(orc, c)[1] > 20


# ---------------------------------------------------------------- the oracle agrees with the restatements
def _bow_cases(ties, depths, weights, sizes, orc):
    """(name, voc, O, desc, levelsup, names) of every transform / vector case."""
    out = [("ties_up%d" % u, ties["voc"], ties["O"], ties["desc"], u, ties["names"]) for u in (0, 1, 2)]
    out += [("depths_up%d" % u, depths["voc"], depths["O"], depths["desc"], u, depths["names"]) for u in range(0, 7)]
    for s, w in COMBOS:
        v = bc.with_scoring(weights["voc"], s, w)
        out.append(("weights_s%d_w%d" % (s, w), v, orc.Vocabulary.from_nodes(v), weights["desc"], 1, weights["names"]))
    O = orc.Vocabulary.from_nodes(sizes["voc"])
    for name, d in sizes["frames"].items():
        out.append(("sizes_" + name, sizes["voc"], O, d, 1, None))
    out.append(("sizes_n1025_up2", sizes["voc"], O, sizes["frames"]["n1025"], 2, None))
    for s, w in ((0, 0), (1, 1), (5, 0), (0, 2)):
        v = bc.with_scoring(sizes["voc"], s, w)
        out.append(("sizes_n257_s%d_w%d" % (s, w), v, orc.Vocabulary.from_nodes(v), sizes["frames"]["n257"], 1, None))
    z = bc.with_zero_weights(sizes["voc"])
    out.append(("sizes_all_zero", z, orc.Vocabulary.from_nodes(z), sizes["frames"]["n17"], 1, None))
    return out


@pytest.fixture(scope="module")
def bow_cases(ties, depths, weights, sizes, orc):
    cases = _bow_cases(ties, depths, weights, sizes, orc)
    return [(c, bc.oracle_bow(c[2], c[3], c[4])) for c in cases]


def test_oracle_equals_numpy_transform_and_vectors(bow_cases):
    for (name, voc, O, desc, levelsup, names), want in bow_cases:
        got = bc.numpy_bow(voc, desc, levelsup)
        bc.same_transform(got, want, names or ["-"] * len(desc), name)
        bc.same_vectors(got, want, name)
        if name == "sizes_all_zero":
            assert len(want["word"]) == 0 and len(want["fv_feature"]) == 0
        if voc["scoring"] != 5 and len(want["word"]):
            v = want["value"]
            assert abs((np.abs(v).sum() if voc["scoring"] != 1 else np.sqrt((v * v).sum())) - 1.0) < 1e-12, name


def test_oracle_equals_numpy_kf_frame(pairs, orc):
    voc, O, g = pairs
    for c in [x for grp in g.values() for x in grp]:
        bc.same_matches(c, bc.numpy_kf_frame(c), bc.oracle_kf_frame(orc, c), "numpy vs oracle")


# ---------------------------------------------------------------- the cases tell every mutant from the oracle
BUILT_FOR = {"last_min": ("ties",), "round_local_tie": ("ties",), "nid_zero_when_unset": ("depths",), "c_times_w": ("weights",),
             "pairwise_norm": ("weights",), "reverse_norm": ("weights",), "keep_zero_weight": ("weights", "sizes"), "sort_by_word_only": ("weights", "sizes"),
             "th_low_exclusive": ("edges",), "ratio_le": ("edges", "tie"), "ignore_taken": ("contention",), "second_best_includes_taken": ("contention",),
             "mask_by_kf_slot": ("masks",), "hist_first_two": ("rotation",), "round_half_even": ("scan",)}


def test_every_mutant_is_caught(bow_cases, pairs, orc, capsys):
    voc, O, g = pairs
    caught = {m: [] for m in bc.TRANSFORM_MUTANTS + bc.VECTOR_MUTANTS + bc.KF_FRAME_MUTANTS}
    for (name, voc_, O_, desc, levelsup, names), want in bow_cases:
        if name.startswith("sizes_") and len(desc) > 300:
            continue                                         # the small frames decide; the restatement is a Python loop per feature
        for m in bc.TRANSFORM_MUTANTS + bc.VECTOR_MUTANTS:
            if bc.differs(bc.numpy_bow(voc_, desc, levelsup, m), want, ALL):
                caught[m].append(name)
    for group, cases in g.items():
        want = [bc.oracle_kf_frame(orc, c) for c in cases]
        for m in bc.KF_FRAME_MUTANTS:
            got = bc.numpy_kf_frame_call(cases, m)
            for c, a, b in zip(cases, got, want):
                if a[1] != b[1] or not np.array_equal(a[0], b[0]):
                    caught[m].append(c["name"])
    with capsys.disabled():
        for m, names in caught.items():
            print("\nmutant %-28s caught by %d cases: %s" % (m, len(names), ", ".join(names[:6]) + (" ..." if len(names) > 6 else "")))
    for m, names in caught.items():
        assert any(n.split("_")[0] in BUILT_FOR[m] or any(n.startswith(b) for b in BUILT_FOR[m]) for n in names), "%s escapes the cases built for it: %r" % (m, names)
    assert all("nodeF_%d" % n in caught["ignore_taken"] for n in (64, 65, 128, 129)), "the taken flags decide at every frame-node size"
    # the weights alone show the three differences of f64 addition, under L1 and under L2
    by = {c[0]: set(m for m in caught if c[0] in caught[m]) for c, _ in bow_cases}
    assert {"c_times_w", "pairwise_norm", "reverse_norm"} <= by["weights_s0_w0"] and {"c_times_w", "pairwise_norm", "reverse_norm"} <= by["weights_s1_w0"]


# ---------------------------------------------------------------- the reference's own classes
def test_vectors_equal_the_reference_classes(bow_cases):
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/libdbow2_ref.so is not built here")
    ref = C.CDLL(REF_SO)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_run = 0
    for (name, voc, O, desc, levelsup, names), want in bow_cases:
        if not (name == "weights_s0_w0" or (name.startswith("sizes_") and voc["scoring"] == 0 and voc["weighting"] == 0)) or not len(desc):
            continue
        n = len(desc)
        word, w, nid = [np.ascontiguousarray(want[f]) for f in ("f_word", "f_weight", "f_node")]
        bw = np.zeros(n, np.uint32); bv = np.zeros(n, np.float64); fn = np.zeros(n, np.uint32); ff = np.zeros(n, np.uint32); nf = C.c_int()
        k = ref.ref_bow_from_features(p(word), p(w), p(nid), n, 1, p(bw), p(bv), p(fn), p(ff), C.byref(nf))
        bc.same_vectors(dict(word=bw[:k], value=bv[:k], fv_node=fn[:nf.value], fv_feature=ff[:nf.value]), want, name + " against DBoW2's classes")
        n_run += 1
    assert n_run >= 15
