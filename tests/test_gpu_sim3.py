"""Sim3Solver RANSAC on the GPU (k_sim3.h through sd_sim3_ransac_host / sd_sim3_ransac_device) against the sequential CPU oracle
tests/cpp/sim3_oracle.cpp: byte equality of every result field and inlier mask on the crafted problems of tests/sim3_cases.py."""
import numpy as np
import pytest

import sim3_cases as sc

pytestmark = pytest.mark.gpu


def _groups():
    """The crafted problems grouped by their RANSAC arguments (one call per group)."""
    g = {}
    for pr in sc.ransac_cases():
        g.setdefault((pr["probability"], pr["min_inliers"], pr["max_iterations"]), []).append(pr)
    return g


def _diff(name, r, inl, ro, io):
    out = []
    for f in sc.RESULT_DTYPE.names:
        if sc.field_bytes(r[f]) != sc.field_bytes(ro[f]):
            out.append("%s.%s: device %r, oracle %r" % (name, f, r[f], ro[f]))
    if inl.tobytes() != io.tobytes():
        out.append("%s: %d inlier bytes differ" % (name, int(np.sum(inl != io))))
    return out


@pytest.fixture(scope="module")
def device_results(gpu, fe):
    """{case name: (result, inliers)} from one sd_sim3_ransac_host call per argument group, plus the packed calls themselves."""
    by, calls = {}, []
    for (prob, mi, mx), prs in _groups().items():
        off, corr, probs = sc.pack(prs)
        res, inl = fe.sim3_ransac(off, corr, probs, prob, mi, mx)
        calls.append(((prob, mi, mx), prs, off, corr, probs, res, inl))
        for k, pr in enumerate(prs):
            by[pr["name"]] = (res[k], inl[off[k]:off[k + 1]])
    return by, calls


def test_problem_ring_and_workspace_over_many_launches_on_two_streams(gpu, fe):
    """sd_sim3_ransac_device on the schedule of solver_ring.py: every output byte of every call equals the problem run alone through the
    host form.  12 .. 57 correspondences: below and above min_inliers = 20."""
    import ctypes as C
    import torch
    import solver_ring as sr
    pool = [sc.make_problem(40 + k, n, outliers=0.3, noise=0.002) for k, n in enumerate(range(12, 60, 3))]
    calls = sr.schedule(pool, lambda pr: len(pr["corr"]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def prepare(prs):
        off, corr, probs = sc.pack(prs)
        return dict(prs=prs, off=off, probs=probs, corr=torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda(),
                    res=torch.full((len(prs) * sc.RESULT_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda"),
                    inl=torch.full((len(corr),), 0x5A, dtype=torch.uint8, device="cuda"))

    def enqueue(a, stream):
        fe.check(fe.lib().sd_sim3_ransac_device(len(a["prs"]), p(a["off"]), dp(a["corr"]), p(a["probs"]), 0.99, 20, 300, dp(a["res"]), dp(a["inl"]),
                                                None, C.c_void_p(stream)))

    done = sr.drive(calls, prepare, enqueue)
    alone = {}
    for k, a in enumerate(done):
        res = a["res"].cpu().numpy().view(sc.RESULT_DTYPE); inl = a["inl"].cpu().numpy(); off = a["off"]
        for q, pr in enumerate(a["prs"]):
            if id(pr) not in alone:
                alone[id(pr)] = fe.sim3_ransac(*sc.pack([pr]), 0.99, 20, 300)
            r, i = alone[id(pr)]
            assert res[q].tobytes() == r[0].tobytes() and inl[off[q]:off[q + 1]].tobytes() == i.tobytes(), (k, q)


def test_every_crafted_problem_gives_the_oracles_bytes(device_results):
    by, _ = device_results
    bad = []
    for pr in sc.ransac_cases():
        ro, io, _ = sc.find(pr)
        r, inl = by[pr["name"]]
        bad += _diff(pr["name"], r, inl, ro, io)
    assert not bad, "%d differences, first: %s" % (len(bad), bad[:6])
    assert len(by) == len(sc.ransac_cases())


def test_alone_equals_beside_others(device_results, fe):
    by, _ = device_results
    for name in ("size_65", "outliers_60", "found_last", "all_outliers", "size_%d" % (sc.LDS_CHUNK + 1)):
        pr = next(p for p in sc.ransac_cases() if p["name"] == name)
        off, corr, probs = sc.pack([pr])
        res, inl = fe.sim3_ransac(off, corr, probs, pr["probability"], pr["min_inliers"], pr["max_iterations"])
        assert sc.same_result(res[0], by[name][0]) and inl.tobytes() == by[name][1].tobytes(), name


def test_host_and_device_forms_agree(device_results, fe):
    _, calls = device_results
    for (prob, mi, mx), prs, off, corr, probs, res, inl in calls:
        r2, i2 = fe.sim3_ransac(off, corr, probs, prob, mi, mx, device=True)
        assert r2.tobytes() == res.tobytes() and i2.tobytes() == inl.tobytes()          # device against device: NaNs included
        for k, pr in enumerate(prs):
            assert res["max_its"][k] == sc.oracle().sd_sim3_oracle_max_its(prob, mi, mx, len(pr["corr"])), pr["name"]
        o_res, o_inl, _ = sc.find_packed(off, corr, probs, prob, mi, mx, threads=3)      # the chunked oracle the bench times
        assert all(sc.same_result(res[k], o_res[k]) for k in range(len(prs))) and inl.tobytes() == o_inl.tobytes()


def test_error_bound_scan_on_the_device(gpu, fe):
    """The 1-ulp scan of the level-0 error bound: every scan value as a problem of its own, all in one call."""
    prs, want = [], []
    for g in range(4):
        pr, row, vals = sc.bound_scan(g, 16)
        for v in vals:
            q = dict(pr, corr=pr["corr"].copy())
            q["corr"]["xw2"][row][0] = v
            prs.append(q)
            want.append(sc.find(q))
    off, corr, probs = sc.pack(prs)
    res, inl = fe.sim3_ransac(off, corr, probs, 0.99, 20, 300)
    flips = 0
    for k, (ro, io, _) in enumerate(want):
        assert sc.same_result(res[k], ro) and inl[off[k]:off[k + 1]].tobytes() == io.tobytes(), k
        flips += int(io[25])
    assert 0 < flips < len(prs)


def test_invalid_tables_are_refused(gpu, fe):
    pr = sc.make_problem(1, 30)
    off, corr, probs = sc.pack([pr])

    def code(*a, **k):
        with pytest.raises(fe.SdError) as e:
            fe.sim3_ransac(*a, **k)
        return e.value.code

    assert code(off, corr, probs, 0.99, 20, 0) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, 0.99, 20, sc.MAX_ITS + 1) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, 0.99, -1, 300) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, 1.0, 20, 300) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, 0.0, 20, 300) == fe.SD_ERR_INVALID
    assert code(off + 1, np.concatenate([corr[:1], corr]), probs, 0.99, 20, 300) == fe.SD_ERR_INVALID      # offsets must start at 0
    big = sc.make_problem(1, sc.MAX_N + 1)
    assert code(*sc.pack([big]), 0.99, 20, 300) == fe.SD_ERR_INVALID                                      # never a truncation
    two = sc.pack([pr, pr])
    dec = two[0].copy(); dec[1], dec[2] = 60, 30
    assert code(dec, two[1], two[2], 0.99, 20, 300) == fe.SD_ERR_INVALID                                   # offsets must not decrease
    many = np.zeros(fe.SIM3_MAX_PROBLEMS + 1, sc.PROBLEM_DTYPE)                                             # a problem is a grid row
    assert code(np.zeros(len(many) + 1, np.int32), corr[:0], many, 0.99, 20, 300) == fe.SD_ERR_INVALID
    res, inl = fe.sim3_ransac(np.zeros(1, np.int32), corr[:0], probs[:0])                                   # no problem: nothing to do
    assert len(res) == 0 and len(inl) == 0


# ---------------------------------------------------------------- SearchBySim3
import fuse_cases as fc          # noqa: E402
import triangulate_cases as tc   # noqa: E402

SLOTS = 8


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = fc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    yield w
    w.close()


def _check_search(ws, scene):
    want, cnt = sc.cpu_search(scene, lv=ws.lv)
    got = sc.device_search(ws, scene)
    sc.assert_same_search(scene, got, want)
    return want, cnt


def test_search_crafted_scene(ws):
    s = sc.crafted_search_scene()
    want, _ = _check_search(ws, s)
    sc.check_search_expectations(s, want)
    assert want[0][3] == 1


@pytest.mark.parametrize("cols", [16, 17])
def test_search_wide_windows(ws, cols):
    s = sc.wide_window_scene(cols)
    want, cnt = _check_search(ws, s)
    assert cnt["cols_max"] == cols


@pytest.mark.parametrize("kind", sc.SEARCH_SCAN_KINDS)
def test_search_scans(ws, kind):
    s, rows = sc.search_scan_scene(kind)
    want, _ = _check_search(ws, s)
    for q, (d, feats, code) in enumerate(rows):
        dec = [int(want[q][4 + d][f]) == code for f in feats]
        assert 0 < sum(dec) < len(dec)


def test_search_random_pairs_in_one_call(ws):
    """Four pairs over eight slots, then the same first pair alone: the result of a pair does not depend on its neighbours."""
    s = sc.random_search_scene(5, 300, 4)
    want, _ = _check_search(ws, s)
    assert sum(w[3] for w in want) > 100
    alone = dict(s, pairs=s["pairs"][:1])
    got = sc.device_search(ws, alone, upload=False)
    sc.assert_same_search(alone, got, want[:1])


def test_search_more_pairs_than_slots_and_growth(gpu, fe, synth):
    """A fresh workspace: one pair, then 11 pairs sharing two slots (the pair tables grow), then the one pair again."""
    w = fc.Workspace(fe, 2, tc.vocabulary(synth, 5))
    try:
        big = sc.random_search_scene(6, 200, 11, slots=(0, 1))
        small = dict(big, pairs=big["pairs"][:1])
        want, _ = sc.cpu_search(big, lv=w.lv)
        sc.assert_same_search(small, sc.device_search(w, small), want[:1])
        sc.assert_same_search(big, sc.device_search(w, big, upload=False), want)
        sc.assert_same_search(small, sc.device_search(w, small, upload=False), want[:1])
    finally:
        w.close()


def test_search_refuses_bad_calls(gpu, fe, synth):
    import torch
    w = fc.Workspace(fe, 2, tc.vocabulary(synth, 5))
    try:
        s = sc.wide_window_scene(16)
        w.upload(s["kfs"])                                                   # key frames written, but no sd_batch_assign_grid
        with pytest.raises(fe.SdError) as e:
            sc.device_search(w, s, upload=False)
        assert e.value.code == fe.SD_ERR_STATE
        want, _ = sc.cpu_search(s, lv=w.lv)
        sc.assert_same_search(s, sc.device_search(w, s), want)
        bad = dict(s, kfs=s["kfs"] * 3, pairs=[dict(s["pairs"][0], k2=5)])                     # a slot the workspace does not have
        with pytest.raises(fe.SdError) as e:
            sc.device_search(w, bad, upload=False)
        assert e.value.code == fe.SD_ERR_INVALID
        with pytest.raises(fe.SdError) as e:
            sc.device_search(w, dict(s, th=0.0), upload=False)
        assert e.value.code == fe.SD_ERR_INVALID
        wild = dict(s, pairs=[dict(s["pairs"][0], p1=s["pairs"][0]["p1"].copy())])
        wild["pairs"][0]["p1"][0] = len(s["points"]) + 7                     # a point index the host cannot see: flagged, never read
        wild["pairs"].append(s["pairs"][0])                                  # a sound pair beside it: the error is the call's
        with pytest.raises(fe.SdError) as e:
            sc.device_search(w, wild, upload=False)
        assert e.value.code == fe.SD_ERR_INVALID
        for pair in (1, 0, 1):                                               # sticky for every pair of that call, in any order
            with pytest.raises(fe.SdError) as e:
                w.b.download_sim3_matches(pair)
            assert e.value.code == fe.SD_ERR_INVALID
        sc.assert_same_search(s, sc.device_search(w, s, upload=False), want)   # the next call starts clean
        torch.cuda.synchronize()
    finally:
        w.close()
