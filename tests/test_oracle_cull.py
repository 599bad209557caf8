"""CPU tests of the crafted cull cases (tests/cull_cases.py) on the oracle's cull half (oracle/cull_oracle.inc): every generator
reaches the branch of Frame::firstSeparate / Tracking::Separate / Frame::UpdateFrame that it is named for, and the oracle itself
agrees with plain numpy restatements of box membership, the empty-box erase, the cross-checked match and (away from the
thresholds) a float64 classifyH / classifyF.  The GPU tests demand the oracle's bytes on the same arrays, so what is pinned here
is what they cover.

Branch pinned per generator:
  membership_edges     every limit of every box has a key point on it and one f32 step outside it; zero / negative extents and boxes
                       outside the image hold nothing; key points in 1, 2, 3 and 64 boxes; bit 63 alone
  empty_box_patterns   all 126 populated / empty patterns of 1 .. 6 boxes, some of which end with an empty box's rectangle and id
                       owning another box's key points; nb = 0; N = 0 with boxes
  partition_sizes      N_s and N_d for N = 1, 255, 256, 257, 511, 513, capacity, first / last key point dynamic or static
  match_sizes          nq x nt as named (a box with fewer than 3 matches is skipped: its matches stay in the scratch list)
  hamming_ties         at least one exact tie per case, the lower index wins, the cross-check rejects
  chunk_boundary       trains beyond 2048, ties across the chunk limit, the nearer train in the later chunk
  match_count_gates    skipped / not skipped as named
  static_count_gates   ret as named
  status_table         box 7's status as named, box 8 keeps -1
  threshold_scans      see test_threshold_scans_see_contraction
  degenerate_models    every match dynamic (epipole: only the match at the epipole)
  readmission          de-duplication, ret 0 with a consistent match
  distortion           a decision that differs between raw and undistorted positions"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cull_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def suite(orc):
    cases = cc.suite()
    return {c["name"]: (c, cc.oracle(orc, c)) for c in cases}


def _kind(suite, kind):
    return [v for v in suite.values() if v[0]["kind"] == kind]


def _lists(r):
    """Box lists of an oracle frame as ORIGINAL key-point indices."""
    return [r["perm"][r["boxItems"][r["boxStart"][b]:r["boxStart"][b + 1]]].tolist() for b in range(len(r["box_idx"]))]


def test_suite_names_and_kinds(suite, orc):
    names = [c["name"] for c in cc.suite()]
    assert len(names) == len(set(names)) == len(suite)
    assert {c["kind"] for c, _ in suite.values()} == {"membership_edges", "empty_box_patterns", "partition_sizes", "match_sizes", "hamming_ties",
                                                      "match_count_gates", "static_count_gates", "status_table", "threshold_scans",
                                                      "degenerate_models", "readmission"}
    assert cc.KP_DTYPE == orc.KP_DTYPE and cc.GEOM.cap == 1272


def test_first_separate_equals_numpy_on_every_frame(suite, orc):
    """Membership (x <= px < x + w in f64 on the f32 position), the stable split, the erase walk and the remapped lists."""
    n_frames = 0
    for c, o in list(suite.values()) + [(c, cc.oracle(orc, c)) for c in cc.distortion()]:
        for side in ("ref", "cur"):
            f, r = c[side], o[side]
            m = cc.np_membership(f["kp"], f["boxes"])
            dyn = m.any(1) if len(f["kp"]) else np.zeros(0, bool)
            assert r["Nd"] == dyn.sum() and r["Ns"] == (~dyn).sum(), c["name"]
            assert r["perm"].tolist() == np.nonzero(~dyn)[0].tolist() + np.nonzero(dyn)[0].tolist(), c["name"]
            exp_kp = f["kp"][r["perm"]].copy(); exp_kp["class_id"][r["Ns"]:] = r["perm"][r["Ns"]:]
            assert r["kp"].tobytes() == exp_kp.tobytes() and np.array_equal(r["desc"], f["desc"][r["perm"]]), c["name"]
            kept, lists = cc.np_first_separate(f)
            assert r["box_idx"].tolist() == [int(f["ids"][j]) for j in kept] and np.array_equal(r["boxes"], f["boxes"][kept].reshape(-1, 4)), c["name"]
            assert _lists(r) == lists, c["name"]
            n_frames += 1
    assert n_frames >= 400


def _gate(ng, nq):
    return ng < 3 or ng < 0.2 * nq


def test_separate_matches_equal_numpy_on_every_box(suite):
    """argmin with first-wins both ways on the descriptors of the two lists, the two count gates, first matching id in the reference."""
    n_boxes = n_matches = 0
    for c, o in suite.values():
        rf, cu = o["ref"], o["cur"]
        lr, lc = _lists(rf), _lists(cu)
        for b, id_ in enumerate(cu["box_idx"]):
            got, _ = cc.box_matches(o, b)
            hit = np.nonzero(rf["box_idx"] == id_)[0]
            if not len(hit) or not lc[b] or not lr[hit[0]]:
                assert len(got) == 0, c["name"]
                continue
            mt, _ = cc.np_crosscheck(c["cur"]["desc"][lc[b]], c["ref"]["desc"][lr[hit[0]]])
            exp = mt[:0] if _gate(len(mt), len(lc[b])) else mt
            assert np.array_equal(got, exp), "%s box %d" % (c["name"], b)
            n_boxes += 1; n_matches += len(exp)
    assert n_boxes > 300 and n_matches > 10000


def test_classification_equals_float64_outside_the_band(suite, orc):
    """Plain float64 classifyH / classifyF (np.linalg.inv, point-to-line distances): where the larger chi-square is <= 0.5 th the match is
    consistent, where it is >= 2 th it is not, and the oracle says the same; inside the band only the oracle speaks.  Every case outside
    threshold_scans and degenerate_models keeps all its matches outside the band (a condition on the inputs, not a tolerance)."""
    n_out = n_in = 0
    for c, o in list(suite.values()) + [(c, cc.oracle(orc, c)) for c in cc.distortion()]:
        B, P1, P2, S = cc.match_points(o, c, orc)
        if not len(B):
            continue
        th = cc.TH_H if c["flag"] == 1 else cc.TH_F
        c1, c2 = cc.chi2_f64(c["M"], c["flag"], P1, P2)
        with np.errstate(invalid="ignore"):
            worst = np.maximum(c1, c2)
            lo, hi = worst <= 0.5 * th, worst >= 2 * th
        assert S[lo].all() and not S[hi].any(), c["name"]
        inside = ~(lo | hi)
        if c["kind"] not in ("threshold_scans", "degenerate_models"):
            assert not inside.any(), "%s: %d matches inside the band" % (c["name"], inside.sum())
        n_out += int((lo | hi).sum()); n_in += int(inside.sum())
    assert n_out > 3000 and n_in > 8000


# ---- branch pins
def test_membership_edges_reach_their_limits(suite):
    c, o = suite["membership_edges-limits"]
    for side in ("ref", "cur"):
        f = c[side]
        m = cc.np_membership(f["kp"], f["boxes"])
        for bi, (x, y, w, h) in enumerate(c["limits"]):
            k = f["kp"][8 * bi:8 * bi + 8]
            px, py = k["x"].astype(np.float64), k["y"].astype(np.float64)
            # first f32 >= the limit and the f32 below it, on the left, right, top and bottom limit
            assert px[0] >= x > px[1] and px[2] >= x + w > px[3] and py[4] >= y > py[5] and py[6] >= y + h > py[7]
            assert m[8 * bi:8 * bi + 8, bi].tolist() == [True, False, False, True, True, False, False, True]
        assert np.float64(np.float32(100.1)) != 100.1 and 0.1 + 0.2 != 0.3
    c, o = suite["membership_edges-degenerate"]
    assert o["cur"]["Nd"] == 6 and len(c["cur"]["ids"]) == 7 and cc.np_membership(c["cur"]["kp"], c["cur"]["boxes"])[:, 1:].sum() == 0
    c, o = suite["membership_edges-whole"]
    assert o["cur"]["Ns"] == 0 and o["cur"]["Nd"] == 12
    c, o = suite["membership_edges-depth"]
    assert sorted(set(cc.np_membership(c["cur"]["kp"], c["cur"]["boxes"]).sum(1).tolist())) == [0, 1, 2, 3, 64]
    assert len(o["cur"]["box_idx"]) == 64 and len(o["appended"]) == 8 and len(o["dyn"]) == 18       # 8 key points re-admitted once each
    c, o = suite["membership_edges-bit63"]
    m = cc.np_membership(c["cur"]["kp"], c["cur"]["boxes"])
    assert m.shape[1] == 64 and m[:, :63].sum() == 0 and m[:, 63].sum() == 8
    assert o["cur"]["boxStart"][1] == 8 and o["cur"]["box_idx"][0] != 263, "an empty box's id owns box 63's key points"


def test_empty_box_patterns_are_exhaustive(suite):
    pats = {c["pattern"] for c, _ in _kind(suite, "empty_box_patterns") if c["pattern"]}
    assert len(pats) == 126 and {len(p) for p in pats} == set(range(1, 7))
    quirk = leading = trailing = run = 0
    for c, o in _kind(suite, "empty_box_patterns"):
        p = c["pattern"]
        if not p:
            continue
        r = o["cur"]
        sizes = np.diff(r["boxStart"])
        # a surviving box with key points whose rectangle belongs to an originally empty box
        quirk += any(sizes[b] > 0 and not p[k] for b, k in enumerate(r["kept_orig"]))
        leading += p[0] == 0 and any(p); trailing += p[-1] == 0 and any(p); run += "00" in "".join(map(str, p)) and any(p)
    assert quirk >= 10 and leading >= 20 and trailing >= 20 and run >= 20, (quirk, leading, trailing, run)
    c, o = suite["empty_box_patterns-001"]                                # the issue's example: [empty, empty, A]
    assert o["cur"]["kept_orig"].tolist() == [1] and o["cur"]["box_idx"].tolist() == [21] and np.diff(o["cur"]["boxStart"]).tolist() == [3]
    c, o = suite["empty_box_patterns-none"]
    assert len(o["cur"]["box_idx"]) == 0 and o["cur"]["Nd"] == 0 and o["ret"] == 0
    for side in ("ref", "cur"):
        c, o = suite["empty_box_patterns-no_keypoints_" + side]
        assert len(c[side]["ids"]) == 2 and len(o[side]["box_idx"]) == 0 and o[side]["Ns"] == o[side]["Nd"] == 0 and len(o["dyn"]) == 0


def test_partition_sizes_reach_their_counts(suite):
    seen = set()
    for c, o in _kind(suite, "partition_sizes"):
        N = len(c["cur"]["kp"])
        seen.add(N)
        assert o["cur"]["Ns"] + o["cur"]["Nd"] == N
        if "alternating" in c["name"]:
            assert o["cur"]["perm"][o["cur"]["Ns"]] == 0 and o["cur"]["perm"][-1] == N - 1 and (N == 1 or o["cur"]["Ns"] >= N // 2 - 1)
        if c["name"].endswith("-static"):
            assert o["cur"]["Nd"] == 0 and len(o["cur"]["box_idx"]) == 0
        if c["name"].endswith("-dynamic"):
            assert o["cur"]["Ns"] == 0 and len(o["appended"]) == N
        if "static_ends" in c["name"]:
            assert o["cur"]["perm"][:2].tolist() == [0, N - 1]
    assert seen == set(cc.PARTITION_SIZES) | {cc.GEOM.cap, 300}


def test_match_sizes_reach_their_sizes(suite):
    got = set()
    for c, o in _kind(suite, "match_sizes"):
        nq, nt = np.diff(o["cur"]["boxStart"])[0], np.diff(o["ref"]["boxStart"])[0]
        assert (nq, nt) == c["sizes"]
        got.add((int(nq), int(nt)))
        n = min(nq, nt)
        assert len(o["dyn"]) == (0 if _gate(n, nq) else n), c["name"]
    assert got == set(cc.MATCH_SIZES) and {(1, 1), (1, 257), (257, 1), (257, 257)} <= got


def _ties(c, o, b=0):
    """(D, row ties, column ties) of current box b against its reference box: a row tie = a query whose minimum is reached twice."""
    lr, lc = _lists(o["ref"]), _lists(o["cur"])
    rb = int(np.nonzero(o["ref"]["box_idx"] == o["cur"]["box_idx"][b])[0][0])
    D = cc.hamming_matrix(c["cur"]["desc"][lc[b]], c["ref"]["desc"][lr[rb]])
    return D, np.nonzero((D == D.min(1, keepdims=True)).sum(1) > 1)[0], np.nonzero((D == D.min(0, keepdims=True)).sum(0) > 1)[0]


def test_hamming_ties_hold_exact_ties(suite):
    for c, o in _kind(suite, "hamming_ties"):
        D, rows, cols = _ties(c, o)
        assert len(rows) + len(cols) >= 1, c["name"]
    c, o = suite["hamming_ties-two_trains_and_cross_check"]
    D, rows, cols = _ties(c, o)
    assert 4 in rows.tolist() and D[4, 2] == D[4, 5] == 20 == D[4].min()
    mt, _ = cc.box_matches(o, 0)
    assert [4, 2] in mt.tolist() and 5 not in mt[:, 1].tolist(), "the lower train wins"
    assert D[7].argmin() == 6 and D[:, 6].argmin() == 6 and 7 not in mt[:, 0].tolist(), "query 7's nearest train prefers query 6"
    for a, b in ((3, 4), (255, 256), (3, 259)):
        c, o = suite["hamming_ties-two_queries_%d_%d" % (a, b)]
        D, rows, cols = _ties(c, o)
        assert a in cols.tolist() and D[a, a] == D[b, a] == 20 == D[:, a].min()
        mt, _ = cc.box_matches(o, 0)
        assert [a, a] in mt.tolist() and b not in mt[:, 0].tolist(), "the lower query wins"
    c, o = suite["hamming_ties-identical"]
    D, rows, cols = _ties(c, o)
    assert (D == 0).all() and D.shape == (8, 8)
    assert len(cc.box_matches(o, 0)[0]) == 0 and cc.np_crosscheck(np.zeros((8, 32), np.uint8), np.zeros((8, 32), np.uint8))[0].tolist() == [[0, 0]], \
        "all distances 0: the one cross-checked match is (0, 0), and a box of one match is skipped"


def test_chunk_boundary_reaches_the_second_chunk(orc):
    cases = {c["name"]: (c, cc.oracle(orc, c)) for c in cc.chunk_boundary(cc.GEOM_BIG.cap)}
    assert cc.GEOM_BIG.cap >= 4200
    for nt in (2047, 2048, 2049, 4097):
        c, o = cases["chunk_boundary-nt%d" % nt]
        assert np.diff(o["ref"]["boxStart"]).tolist() == [nt]
        mt, dyn = cc.box_matches(o, 0)
        assert mt[:len(c["partners"]), 1].tolist() == c["partners"] and (dyn != -1).all() and c["partners"][-1] == nt - 1
        ref_mt, _ = cc.np_crosscheck(o["cur"]["desc"][o["cur"]["Ns"]:], o["ref"]["desc"][o["ref"]["Ns"]:])
        assert np.array_equal(mt, ref_mt)
    c, o = cases["chunk_boundary-nt4097"]
    D, rows, cols = _ties(c, o)
    mt, _ = cc.box_matches(o, 0)
    n = len(c["partners"])
    assert rows.tolist() == [n, n + 1] and mt[n:].tolist() == [[n, 2047], [n + 1, 100], [n + 2, 2100]]
    assert D[n, 2047] == D[n, 2048] == 20 and D[n + 1, 100] == D[n + 1, 2148] == 20 and D[n + 2, 50] == 30 and D[n + 2, 2100] == 10


def test_match_count_gates_skip_as_named(suite):
    seen = []
    for c, o in _kind(suite, "match_count_gates"):
        nq, ng = c["gate"]
        assert np.diff(o["cur"]["boxStart"]).tolist() == [nq, 6]
        mt0, _ = cc.box_matches(o, 0); mt1, _ = cc.box_matches(o, 1)
        assert len(mt0) == (0 if c["skipped"] else ng) and len(mt1) == 6, c["name"]
        seen.append((nq, ng, c["skipped"]))
    assert seen == [(2, 2, True), (3, 3, False), (15, 3, False), (16, 3, True), (50, 10, False), (51, 10, True)]


def test_static_count_gates_return_as_named(suite):
    seen = []
    for c, o in _kind(suite, "static_count_gates"):
        ng, num0 = c["gate"]
        _, dyn = cc.box_matches(o, 0)
        assert len(dyn) == ng and (dyn != -1).sum() == num0 and o["ret"] == int(c["static"]), c["name"]
        assert o["status"].tolist() == ([-1] if c["static"] else [0])
        seen.append((ng, num0, o["ret"]))
    assert seen == [(3, 1, 0), (3, 2, 1), (10, 2, 0), (10, 3, 1), (11, 2, 0), (11, 3, 1), (5, 1, 0), (5, 2, 1)]
    assert {c["flag"] for c, _ in _kind(suite, "static_count_gates")} == {1, 2}


def test_status_table_ends_as_named(suite):
    got = {}
    for c, o in _kind(suite, "status_table"):
        ids = o["cur"]["box_idx"].tolist()
        assert o["status"][ids.index(8)] == -1 and o["ret"] == 1, c["name"]
        if c["expect"] is None:
            assert 7 not in ids
        else:
            assert o["status"][ids.index(7)] == c["expect"], c["name"]
        got[c["name"].split("-")[1]] = c["expect"]
    assert got == dict(absent=0, last_m1=0, last_0=2, last_1=0, last_2=2, twice_0_then_1=2, twice_1_then_0=0, n_last_0=0, n_last_64=2,
                       absent_from_ref=-1, twice_in_ref=-1, no_keypoints_ref=-1, no_keypoints_cur=None)
    c, o = suite["status_table-twice_in_ref"]
    assert o["ref"]["box_idx"].tolist().count(7) == 2 and (cc.box_matches(o, 0)[1] != -1).all()
    c, o = suite["status_table-n_last_64"]
    assert len(c["last_idx"]) == 64 and c["last_idx"][63] == 7


def test_degenerate_models_end_dynamic(suite):
    for c, o in _kind(suite, "degenerate_models"):
        _, dyn = cc.box_matches(o, 0)
        assert len(dyn) == 10
        if c["all_dynamic"]:
            assert (dyn == -1).all() and o["ret"] == 0 and o["status"].tolist() == [2], c["name"]
        else:
            assert c["name"].endswith("epipole") and dyn.tolist() == [-1] + list(range(1, 10))
    assert len(_kind(suite, "degenerate_models")) == 10


def test_readmission_deduplicates_and_keeps_ret0(suite, orc):
    c, o = suite["readmission-shared"]
    cu = o["cur"]
    assert o["ret"] == 1 and (o["dyn"] != -1).all() and len(o["dyn"]) == 14 and len(o["appended"]) == 11
    cid = cu["kp"]["class_id"][o["appended"]]
    assert cid.tolist() == [c0 + 4 for c0 in range(7)] + [c0 + 4 for c0 in range(7, 11)], "shared key points at box 1's position, once"
    c, o = suite["readmission-ret0"]
    assert o["ret"] == 0 and (o["dyn"] != -1).sum() == 1 and len(o["appended"]) == 1
    assert len(cc.oracle(orc, c, only_if_static=True)["kp_after"]) == o["cur"]["Ns"] == len(o["kp_after"]) - 1


def test_distortion_changes_a_decision(orc):
    (c,) = cc.distortion()
    o = cc.oracle(orc, c)
    raw = cc.oracle(orc, dict(c, dist=False))
    assert np.array_equal(o["matches"], raw["matches"]) and len(o["dyn"]) == 24
    assert (o["dyn"] != -1).all() and (raw["dyn"] == -1).sum() >= 1, "consistent in mvKeysUn, %d of 24 inconsistent in the raw positions" % (raw["dyn"] == -1).sum()
    un = cc._un(orc, c["cur"]["kp"])
    assert np.abs(un["x"] - c["cur"]["kp"]["x"]).max() > 2.0


# ---- the thresholds
def _scan_arrays(c, o):
    """-> (ref_xy, cur_xy, identity matches, oracle decisions, [(first, length)] scans) over all boxes of a threshold_scans case."""
    B, P1, P2, S = cc.match_points(o, c)
    first = np.concatenate([[0], np.cumsum(np.diff(o["dynStart"]))])
    for b in range(len(o["cur"]["box_idx"])):
        mt, _ = cc.box_matches(o, b)
        assert np.array_equal(mt, np.stack([np.arange(len(mt))] * 2, 1)), "%s: every match of box %d is an intended one" % (c["name"], b)
    scans = [(int(first[b]) + off, n) for b, off, n in c["scans"]]
    return P1, P2, S, scans


def _classify(L, M, flag, P1, P2):
    n = len(P1)
    mt = np.ascontiguousarray(np.stack([np.arange(n)] * 2, 1), np.int32); out = np.zeros(n, np.int32)
    M = np.ascontiguousarray(M, np.float32).reshape(9); a = np.ascontiguousarray(P2, np.float32); b = np.ascontiguousarray(P1, np.float32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    L.orc_classify(p(M), C.c_int(flag), p(a), p(b), p(mt), C.c_int(n), p(out))
    return out != -1


@pytest.fixture(scope="module")
def contracted(tmp_path_factory):
    """oracle/sd_oracle.cpp once more, with contraction allowed."""
    with open("/proc/cpuinfo") as f:
        if " fma" not in f.read():
            pytest.skip("the host CPU has no FMA: a contracted build cannot run here")
    so = str(tmp_path_factory.mktemp("contracted") / "libsd_oracle_fma.so")
    subprocess.check_call(["g++", "-O3", "-march=x86-64-v3", "-ffp-contract=fast", "-fno-fast-math", "-fPIC", "-std=c++17", "-shared", "-o", so,
                           os.path.join(ROOT, "oracle", "sd_oracle.cpp")])
    return C.CDLL(so)


@pytest.mark.parametrize("flag", [1, 2])
def test_threshold_scans_see_contraction(suite, orc, contracted, flag):
    """The scans sit on the threshold: under the oracle (built with -ffp-contract=off, like the library) most scans hold both outcomes, and the
    same source built with -ffp-contract=fast decides many of their matches differently, so a contraction or re-association in the device
    code would change bytes that the GPU test compares.  Measured when written: flag 1: 4,556 matches in 268 scans, all 268 scans hold both
    outcomes, 112 decisions differ under contraction; flag 2: 4,352 matches in 256 scans, all 256 scans hold both outcomes, 95 decisions
    differ.  The floors are the issue's: 50 decisions, 80 % of the scans."""
    n = both = differ = nscans = 0
    for c, o in _kind(suite, "threshold_scans"):
        if c["flag"] != flag:
            continue
        P1, P2, S, scans = _scan_arrays(c, o)
        ours = _classify(orc.lib(), c["M"], flag, P1, P2)
        assert np.array_equal(ours, S), "orc_classify alone decides as orc_separate does"
        fma = _classify(contracted, c["M"], flag, P1, P2)
        n += len(S); differ += int((ours != fma).sum()); nscans += len(scans)
        both += sum(1 for s0, ln in scans if 0 < S[s0:s0 + ln].sum() < ln)
    print("threshold_scans flag %d: %d matches in %d scans, %d scans hold both outcomes, %d decisions differ under contraction" % (flag, n, nscans, both, differ))
    assert nscans >= 200 and differ >= 50 and both >= 0.8 * nscans, (nscans, both, differ)


def test_exact_threshold_variant_is_exact(suite):
    """H = I, v1 == v2: u1 - u2 is exact, the inverse is exact, so chi-square is fl(d * d) and the decision is fl(d * d) <= fl(5.991)."""
    c, o = suite["threshold_scans-flag1-exact"]
    B, P1, P2, S = cc.match_points(o, c)
    d = (P1[:, 0].astype(np.float64) - P2[:, 0].astype(np.float64))
    assert np.array_equal(d, (P1[:, 0] - P2[:, 0]).astype(np.float64)) and (P1[:, 1] == P2[:, 1]).all()
    assert np.array_equal(S, np.float32(d * d) <= np.float32(5.991)) and 0 < S.sum() < len(S)
    for s0, ln in _scan_arrays(c, o)[3]:
        assert 0 < S[s0:s0 + ln].sum() < ln
