"""GPU parity of k_bow_transform, k_bow_finalize (sd_batch_compute_bow) and k_search_by_bow (sd_batch_search_by_bow) with the oracle on
the crafted trees, descriptors and pairs of bow_cases.py: every comparison is byte for byte (f64 values as their bits), and a
difference is reported with the feature it first shows at and what that feature was built for.  test_bow_cases.py shows on the CPU that
the inputs hold what they claim and that they tell each deliberate error of the restatements from the oracle."""
import numpy as np
import pytest

import bow_cases as bc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SLOTS = 8


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = bc.workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    yield w
    bc.close_workspace(w)


@pytest.fixture(scope="module")
def big(gpu, fe, synth):
    """The workspace whose rows hold 1025 key points."""
    w = bc.workspace(fe, SLOTS, tc.vocabulary(synth, 5), big=True)
    assert 1025 <= w.cap <= 2048
    yield w
    bc.close_workspace(w)


@pytest.fixture(scope="module")
def pairs(synth, orc):
    voc = tc.vocabulary(synth, 5)
    O = orc.Vocabulary.from_nodes(voc)
    voc, groups = bc.kf_frame_cases(synth, orc, O)
    return voc, O, groups


@pytest.fixture(scope="module")
def sizes(orc):
    g = bc.sizes()
    g["O"] = orc.Vocabulary.from_nodes(g["voc"])
    return g


def _check_bow(ws, fe, orc, voc, frames, levelsup, names=None, what="", O=None):
    """One compute_bow call over `frames` against the oracle -> (features, words, listed features) summed over the frames."""
    V = fe.Vocabulary.from_nodes(voc)
    O = O or orc.Vocabulary.from_nodes(voc)
    try:
        got = bc.device_compute_bow(ws, V, frames, levelsup)
    finally:
        V.close()
    tot = [0, 0, 0]
    for j, (g, d) in enumerate(zip(got, frames)):
        want = bc.oracle_bow(O, d, levelsup)
        tag = "%s frame %d levelsup %d" % (what, j, levelsup)
        bc.same_transform(g, want, names[j] if names else ["-"] * len(d), tag)
        bc.same_vectors(g, want, tag)
        tot[0] += len(d); tot[1] += len(want["word"]); tot[2] += len(want["fv_feature"])
    return tuple(tot)


# ---------------------------------------------------------------- Frame::ComputeBoW
def test_transform_ties_and_depths(ws, fe, orc):
    """Per feature word, weight bits and node: equal distances inside a 16-lane round and across the two, at both levels; distance 256;
    16-lane groups of one wave that leave the descent after 1, 2, 3 and 5 rounds; nid at every levelsup from 0 to L + 1."""
    t = bc.ties()
    rev = t["desc"][::-1].copy()
    for u in (0, 1, 2, 3):
        n = _check_bow(ws, fe, orc, t["voc"], [t["desc"], rev], u, [t["names"], t["names"][::-1]], "ties")
    print("\nties: 2 frames x %d features at levelsup 0..3, %d words; cases %s" % (len(t["desc"]), n[1], ", ".join(t["names"])))
    d = bc.depths()
    for u in range(0, d["voc"]["L"] + 2):
        n = _check_bow(ws, fe, orc, d["voc"], [d["desc"], d["desc"][:37]], u, [d["names"], d["names"][:37]], "depths")
    print("depths: frames of 64 and 37 features at levelsup 0..%d, %d words; cases %s" % (d["voc"]["L"] + 1, n[1], ", ".join(sorted(set(d["names"])))))


def test_vectors_all_scorings(ws, fe, orc):
    """The `weights` frame (words hit 1, 2, 3, 5, 7 and 70 times in interleaved order, weights over 12 decades, weightless words) under
    every scoring and weighting: the values bit for bit."""
    g = bc.weights()
    n = None
    for s in range(6):
        for w in range(4):
            n = _check_bow(ws, fe, orc, bc.with_scoring(g["voc"], s, w), [g["desc"]], 1, [g["names"]], "weights scoring %d weighting %d" % (s, w))
    print("\nweights: 24 vocabularies x %d features, %d words, %d listed features; hits %r" % (n[0], n[1], n[2], bc.HITS))


def test_vector_sizes(big, fe, orc, sizes):
    """Every N at which k_bow_finalize changes its sort size or its per-thread chunk, 64 / 65 words, one word, no weight at all."""
    names = list(sizes["frames"])
    frames = [sizes["frames"][k] for k in names]
    tot = [0, 0, 0]
    for i in range(0, len(frames), SLOTS):
        n = _check_bow(big, fe, orc, sizes["voc"], frames[i:i + SLOTS], 1, None, "sizes " + "/".join(names[i:i + SLOTS]), sizes["O"])
        tot = [a + b for a, b in zip(tot, n)]
    last = [sizes["frames"][k] for k in ("n1025", "n513", "n257", "n1")]
    _check_bow(big, fe, orc, sizes["voc"], last, 2, None, "sizes, one run (levelsup = L)", sizes["O"])
    for s, w in ((1, 1), (5, 0), (0, 2), (4, 3)):
        _check_bow(big, fe, orc, bc.with_scoring(sizes["voc"], s, w), [sizes["frames"]["n257"], sizes["frames"]["n1025"]], 1, None, "sizes scoring %d weighting %d" % (s, w))
    n = _check_bow(big, fe, orc, bc.with_zero_weights(sizes["voc"]), [sizes["frames"]["n17"], sizes["frames"]["n513"]], 1, None, "sizes, every weight 0")
    assert n[1] == 0 and n[2] == 0
    print("\nsizes: %s; sort sizes %r; %d features, %d words, %d listed features" % (", ".join(names), sorted(set(bc.sort_size(x)[0] for x in bc.SIZES)), tot[0], tot[1], tot[2]))


def test_slot_history_and_selection(big, fe, orc, sizes):
    """A slot's result does not depend on what the slot held before, nor on the order of the slots in the call, and a call leaves the
    other slots' vectors as they were."""
    V = fe.Vocabulary.from_nodes(sizes["voc"]); O = sizes["O"]
    fr = sizes["frames"]
    try:
        for first, second in (("n1025", "n17"), ("n17", "n1025")):
            bc.device_compute_bow(big, V, [fr[first]], 1, slots=[3])
            got, = bc.device_compute_bow(big, V, [fr[second]], 1, slots=[3])
            want = bc.oracle_bow(O, fr[second], 1)
            bc.same_transform(got, want, ["-"] * len(fr[second]), "%s after %s" % (second, first)); bc.same_vectors(got, want, "%s after %s" % (second, first))
        base = bc.device_compute_bow(big, V, [fr["n%d" % n] for n in (15, 16, 257, 1, 513, 255, 17, 512)], 1)
        a = bc.device_compute_bow(big, V, [fr["nb65"], fr["n1024"]], 1, slots=[5, 2])
        others = {s: big.b.download_bow(s) for s in (0, 1, 3, 4, 6, 7)}
        for s, g in others.items():
            assert not bc.differs(g, base[s], tuple(g)), "slot %d changed under a call on slots 5 and 2" % s
        b = bc.device_compute_bow(big, V, [fr["n1024"], fr["nb65"]], 1, slots=[2, 5])
        for x, y, name in ((a[0], b[1], "nb65"), (a[1], b[0], "n1024")):
            assert not bc.differs(x, y, tuple(x)), "%s: [5, 2] and [2, 5] differ" % name
            bc.same_vectors(x, bc.oracle_bow(O, fr[name], 1), name)
    finally:
        V.close()
    print("\nslot history: 1025 -> 17 -> 1025 in one slot; [5, 2] against [2, 5]; six bystanders unchanged")


# ---------------------------------------------------------------- SearchByBoW(KeyFrame*, Frame&, ...)
def _check_pairs(ws, orc, cases, slots=None, what=""):
    got = bc.device_kf_frame(ws, cases, slots)
    nm = 0
    for c, g in zip(cases, got):
        bc.same_matches(c, g, bc.oracle_kf_frame(orc, c), what)
        bc.check_expect(c, g[0])
        nm += g[1]
    return nm


def test_kf_frame_named_cases(ws, orc, pairs):
    """Distance 50 / 51, both sides of the ratio edge at 0.7 and 0.75, a single candidate, the mask, nodes of one side only at both ends
    of the frame's list, 20 shared nodes, no mask, ties, contention across a 64-block and in the second register slot, frame nodes of
    64 / 65 / 128 / 129, empty sides, one keyframe under two mask rows -- then every call again with its pairs reversed and the
    keyframes in the odd slots."""
    voc, O, g = pairs
    cases = [c for name in ("edges", "tie", "contention", "node_sizes", "empty") for c in g[name]]
    total = 0
    for part in bc.call_groups(cases):
        total += _check_pairs(ws, orc, part, None, "in order")
        back = part[::-1]
        _check_pairs(ws, orc, back, [(2 * q + 1, 2 * q) for q in range(len(back))][::-1], "reversed")
    m = g["masks"]
    total += _check_pairs(ws, orc, m, [(0, 1), (0, 2)], "masks")
    _check_pairs(ws, orc, m[::-1], [(6, 3), (6, 5)], "masks reversed")
    print("\nkf-frame: %d pairs, %d matches; cases %s" % (len(cases) + 2, total, ", ".join(c["name"] for c in cases + m)))


def test_kf_frame_orientation(ws, orc, pairs):
    """Three equal maxima, a removed bin, bin == 30, rot < 0; max2 against a tenth of max1 on both sides; 16 consecutive f32 angles
    across the edge of bin 0; all of it with the check off as well."""
    voc, O, g = pairs
    cases = g["rotation"] + g["scan"]
    off = []
    for c in g["rotation"][2:] + g["scan"]:
        o = dict(c); o.update(name=c["name"] + "_off", check_orientation=False, expect={})
        off.append(o)
    total = 0
    for part in bc.call_groups(cases + off):
        total += _check_pairs(ws, orc, part, None, "orientation")
    print("\nkf-frame orientation: %d pairs, %d matches; cases %s" % (len(cases + off), total, ", ".join(c["name"] for c in cases + off)))


def test_kf_frame_random(ws, orc, pairs):
    voc, O, g = pairs
    cases = [bc.random_case(voc, O, s, r, m) for s in (0, 1, 2) for r in (0.7, 0.75) for m in (True, False)]
    total = 0
    for part in bc.call_groups(cases):
        total += _check_pairs(ws, orc, part, None, "random")
    assert total > 20 * len(cases)                           # test_bow_cases.py: every such pair has more than 20 matches
    print("\nkf-frame random: %d pairs of about 260 points, %d matches" % (len(cases), total))


def test_refusals(fe, synth, gpu):
    """Both refusals come from the host before anything is launched: the slots keep the state they had."""
    voc = tc.vocabulary(synth, 5)
    w2 = tc.Workspace(fe, 2, voc)
    try:
        with pytest.raises(fe.SdError) as e:
            w2.b.search_by_bow([0], [1], 0.75, True)
        assert e.value.code == fe.SD_ERR_STATE
        w2.b.compute_bow(w2.V, [0], tc.LEVELSUP)
        with pytest.raises(fe.SdError) as e:
            w2.b.search_by_bow([0], [1], 0.75, True)        # the frame's slot still has none
        assert e.value.code == fe.SD_ERR_STATE
        with pytest.raises(fe.SdError) as e:
            w2.b.download_bow(1)
        assert e.value.code == fe.SD_ERR_STATE
    finally:
        w2.close()
    ex = fe.ORBextractor(8300, 1.2, 8, 20, 7)
    b = fe.Batch(ex, tc.GEOM["W"], tc.GEOM["H"], 1)
    V = fe.Vocabulary.from_nodes(voc)
    try:
        assert b.cap > 8192
        b.extract_host(np.full((1, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); b.sync()
        with pytest.raises(fe.SdError) as e:
            b.compute_bow(V, [0], tc.LEVELSUP)
        assert e.value.code == fe.SD_ERR_UNSUPPORTED
        with pytest.raises(fe.SdError) as e:
            b.download_bow(0)
        assert e.value.code == fe.SD_ERR_STATE, "nothing was computed for the slot"
    finally:
        V.close(); b.close()
