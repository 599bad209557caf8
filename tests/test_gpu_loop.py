"""GPU parity of sd_batch_search_by_bow_kf / sd_batch_search_by_projection_sim3 / sd_batch_fuse_sim3 with the sequential CPU oracle
(tests/cpp/loop_oracle.cpp): every crafted case of loop_cases.py, the 1-ulp scans, the shapes at which the kernels take another path,
seeded random scenes, the independence of a job from its launch, and the refusals -- all byte for byte."""
import ctypes as C

import numpy as np
import pytest

import fuse_cases as fc
import loop_cases as lc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SLOTS = 8


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = lc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    assert fc.inv_sigma2(w.lv).tobytes() == w.ex.mvInvLevelSigma2.tobytes()
    yield w
    w.close()


@pytest.fixture(scope="module")
def bow(synth, orc):
    O = orc.Vocabulary.from_nodes(tc.vocabulary(synth, 5))
    voc, cases = lc.bow_cases(synth, O)
    return voc, O, cases


@pytest.fixture(scope="module")
def crafted():
    return lc.crafted_scene()


def check_fuse(ws, scene, upload=True):
    want, _ = lc.cpu_fuse(scene, lv=ws.lv)
    fc.assert_same(scene, lc.device_fuse(ws, scene, upload=upload), want)
    return want


def check_project(ws, scene, upload=True):
    want, _ = lc.cpu_project(scene, lv=ws.lv)
    lc.assert_same_project(scene, lc.device_project(ws, scene, upload=upload), want)
    return want


# ---------------------------------------------------------------- Fuse(pKF, Scw, ...) and SearchByProjection(pKF, Scw, ...)
@pytest.mark.parametrize("scale", lc.SCALES)
def test_crafted_cases_at_every_scale(ws, crafted, scale):
    """The shared search cases, the four actions, the member at distance 256 and the level gate, through both functions."""
    sc = lc.with_scale(crafted, scale)
    sc["matched"] = lc.matched_from_state(sc); sc["th_proj"] = 3
    want = check_fuse(ws, sc)
    if scale == 1.0:
        lc.check_crafted(sc, want)
    pw = check_project(ws, sc, upload=False)
    assert sum(w[2] for w in pw) > 10


def test_crafted_projection_cases(ws):
    """spAlreadyFound, targets matched on entry, two / three / 65 candidates on one feature, the chain, positions 63 / 64."""
    sc = lc.projection_scene()
    want = check_project(ws, sc)
    lc.check_projection(sc, want)


def test_v_on_the_lower_image_bound(ws):
    """v == mnMinY exactly (a camera with cy = fy / 4): inside through both functions, the next float outside."""
    sc = lc.v_min_scene()
    want, br = lc.cpu_fuse(sc, cam=lc.CAM_VMIN, lv=ws.lv)
    assert br["v_eq_miny"] == 1 and tuple(want[0][0][0]) == (0, 10) and tuple(want[0][0][1]) == (-1, 256)
    fc.assert_same(sc, lc.device_fuse(ws, sc, cam=lc.CAM_VMIN), want)
    pw, _ = lc.cpu_project(sc, cam=lc.CAM_VMIN, lv=ws.lv)
    assert pw[0][2] == 1
    lc.assert_same_project(sc, lc.device_project(ws, sc, cam=lc.CAM_VMIN, upload=False), pw)


@pytest.mark.parametrize("cols", [16, 17])
def test_window_of_16_and_17_columns(ws, cols):
    sc = lc.with_scale(lc.wide_window_scene(cols), 1.0)
    (best, hits, nf), = check_fuse(ws, sc)
    assert tuple(best[0]) == (39, 9) and nf == 1
    (assigned, pbest, nm), = check_project(ws, sc, upload=False)
    assert nm == 1 and assigned[39] == 0


def test_scale_one_equals_the_plain_fuse(ws):
    """Scale 1 over a pose the decomposition returns bit for bit, every feature passing the chi-square test: sd_batch_fuse_sim3 gives
    the bytes of sd_batch_fuse."""
    sc = lc.rigid_exact_scene()
    want = check_fuse(ws, sc)
    plain = fc.device_run(ws, sc, upload=False)
    fc.assert_same(sc, plain, want)
    assert want[0][2] > 50


@pytest.mark.parametrize("kind", lc.SCAN_KINDS)
def test_threshold_scans(ws, kind):
    sc = lc.scan_scene(kind)
    sc["th_proj"] = int(sc.get("th", 3.0))
    (best, hits, nf), = check_fuse(ws, sc)
    assert 0 < nf < 512
    check_project(ws, sc, upload=False)


@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(ws, seed):
    """4 jobs x 240 candidates over 200 features, scales 1 / 0.5 / 2 / 1.37 by seed, feature states, candidates already found."""
    sc = lc.random_scw_scene(seed)
    want = check_fuse(ws, sc)
    assert sum(w[2] for w in want) > 50
    pw = check_project(ws, sc, upload=False)
    assert sum(w[2] for w in pw) > 50


def test_a_job_does_not_depend_on_its_launch(ws):
    """The jobs of a scene alone, reversed and repeated: each gives the bytes it gives in the full call."""
    sc = lc.random_scw_scene(3)
    fw = check_fuse(ws, sc)
    pw = check_project(ws, sc, upload=False)
    for order in ([2], [3, 2, 1, 0], [1, 1, 0, 3, 3, 2, 0]):
        sub = dict(sc)
        sub["jobs"] = [sc["jobs"][q] for q in order]; sub["scw"] = [sc["scw"][q] for q in order]; sub["matched"] = [sc["matched"][q] for q in order]
        fc.assert_same(sub, lc.device_fuse(ws, sub, upload=False), [fw[q] for q in order])
        lc.assert_same_project(sub, lc.device_project(ws, sub, upload=False), [pw[q] for q in order])


def test_job_sizes(ws):
    """Jobs of 0, 1, 63, 64, 65 and 257 entries in one call."""
    sc = lc.with_scale(fc.sized_jobs_scene(), 1.37)
    sc["matched"] = lc.matched_from_state(sc)
    want = check_fuse(ws, sc)
    assert [len(w[0]) for w in want] == [0, 1, 63, 64, 65, 257]
    check_project(ws, sc, upload=False)


def test_projection_tables_grow_with_a_larger_second_call(gpu, fe, synth):
    """A fresh workspace: one job of one candidate, then 4 jobs of 120 candidates each (the job and the entry tables both grow), then the
    first call again."""
    w = lc.Workspace(fe, 4, tc.vocabulary(synth, 5))
    try:
        small = lc.with_scale(fc.contention_scene(1), 1.0)
        small["th_proj"] = 3
        big = lc.random_scw_scene(1)
        assert len(big["jobs"]) == 4 and sum(len(j[1]) for j in big["jobs"]) == 480
        for sc in (small, big, small):
            check_project(w, sc)
    finally:
        w.close()


def test_all_candidates_contend_for_one_feature(ws):
    sc = lc.with_scale(fc.contention_scene(40), 2.0)
    (best, hits, nf), = check_fuse(ws, sc)
    assert nf == 40 and int((hits["action"] == fc.ADD).sum()) == 1 and int((hits["action"] == fc.MEET_CANDIDATE).sum()) == 39
    (assigned, pbest, nm), = check_project(ws, sc, upload=False)
    assert nm == 1 and int((pbest[:, 0] >= 0).sum()) == 1


def test_list_bound_is_reported_not_guessed(ws, fe):
    """70 features within TH_LOW of 66 identical candidates: the 65th finds its 64 kept keys taken while the window held 70.  The oracle
    has an answer (the 65th feature); the library refuses the call's results, and the next call is clean."""
    S = fc.SceneBuilder(950)
    A = S.keyframe(tc.T1_DEFAULT)
    d0 = fc.rand_desc(S.rng)
    for j in range(70):
        S.kfs[A].add(400.0 + 0.05 * j, 200.0, fc.flipped(d0, j % 40, S.rng), 2)
    S.job(A, [S.point(A, 401.0, 200.0, 10.0, 2, desc=d0) for _ in range(66)])
    sc = lc.with_scale(S.build("list_bound"), 1.0)
    sc["th_proj"] = 3
    want, _ = lc.cpu_project(sc, lv=ws.lv)
    assert want[0][2] == 66
    with pytest.raises(fe.SdError) as e:
        lc.device_project(ws, sc)
    assert e.value.code == fe.SD_ERR_UNSUPPORTED
    sc["jobs"] = [(A, sc["jobs"][0][1][:64], None)]
    (assigned, best, nm), = check_project(ws, sc)
    assert nm == 64


# ---------------------------------------------------------------- SearchByBoW(pKF1, pKF2, ...)
def test_crafted_bow_cases(ws, bow):
    """Every crafted pair, four pairs per call where the matcher's settings agree."""
    _, _, cases = bow
    groups = {}
    for c in cases.values():
        groups.setdefault((c["nnratio"], c["check_orientation"]), []).append(c)
    for group in groups.values():
        for i in range(0, len(group), SLOTS // 2):
            part = group[i:i + SLOTS // 2]
            got = lc.device_bow(ws, part)
            for c, (m, nm) in zip(part, got):
                wm, wn, _ = lc.cpu_bow(c)
                assert nm == wn and m.tobytes() == wm.tobytes(), "%s: %r vs %r" % (c["name"], m, wm)
                for a, b in c["expect"].items():
                    assert int(m[a]) == b, c["name"]


@pytest.mark.parametrize("seed", range(8))
def test_random_bow_pairs(ws, bow, seed):
    voc, O, _ = bow
    c = lc.random_bow_case(voc, O, seed)
    (m, nm), = lc.device_bow(ws, [c])
    wm, wn, _ = lc.cpu_bow(c)
    assert nm == wn and m.tobytes() == wm.tobytes() and nm > 5


def test_bow_pair_does_not_depend_on_its_launch(ws, bow):
    voc, O, _ = bow
    cs = [lc.random_bow_case(voc, O, s) for s in (1, 3, 5, 7)]          # one nnratio, one orientation switch
    cs = [c for c in cs if (c["nnratio"], c["check_orientation"]) == (cs[0]["nnratio"], cs[0]["check_orientation"])]
    assert len(cs) >= 2
    alone = [lc.device_bow(ws, [c])[0] for c in cs]
    for got, want in zip(lc.device_bow(ws, cs[::-1]), alone[::-1]):
        assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes()


# ---------------------------------------------------------------- refusals
def test_out_of_table_match_on_a_feature_no_candidate_visits(ws, fe):
    """The row scan reports a d_matched value outside the table wherever it sits; the same call with the value in range is answered."""
    S = fc.SceneBuilder(960)
    A = S.keyframe(tc.T1_DEFAULT)
    p = S.point(A, 300.0, 150.0, 10.0, 2)
    S.feature(A, 300.0, 150.0, p, 10); S.kfs[A].add(1100.0, 340.0, fc.rand_desc(S.rng), 2)
    S.job(A, [p])
    sc = lc.with_scale(S.build("far_bad_match"), 1.0)
    sc["th_proj"] = 3
    for bad in (len(sc["points"]), -3):
        sc["matched"] = [np.array([-1, bad], np.int32)]
        with pytest.raises(fe.SdError) as e:
            lc.device_project(ws, sc)
        assert e.value.code == fe.SD_ERR_INVALID
    sc["matched"] = [np.array([-1, -2], np.int32)]
    (assigned, best, nm), = check_project(ws, sc)
    assert nm == 1 and assigned[0] == 0


def test_refusals(ws, fe, synth):
    import torch
    sc = lc.with_scale(fc.contention_scene(5), 1.0)
    ws.upload_grid([sc["kfs"][0], sc["kfs"][0]])
    lc.device_fuse(ws, sc, upload=False)
    L, b = fe.lib(), ws.b
    cam = fe.camera_array(tc.CAM)
    pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda()
    desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
    ent = torch.from_numpy(sc["jobs"][0][1].copy()).cuda()
    matched = torch.full((2, ws.cap), -1, dtype=torch.int32).cuda()
    S = np.ascontiguousarray(sc["scw"][0], np.float32).reshape(16)
    out = [C.c_void_p(), C.c_void_p(), C.c_void_p()]

    def fuse(n_jobs=1, kf=(0,), off=(0, 5), th=3.0, tables=True, entries=ent):
        k = np.array(kf, np.int32); o = np.array(off, np.int32)
        return L.sd_batch_fuse_sim3(b.h, n_jobs, fc._p(k) if tables else None, fc._p(S) if tables else None, fc._p(o) if tables else None,
                                    C.c_void_p(entries.data_ptr()), C.c_void_p(pts.data_ptr()), C.c_void_p(desc.data_ptr()), 5, None,
                                    fc._p(cam), C.c_float(th), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), None)

    def proj(n_jobs=1, kf=(0,), off=(0, 5), th=3, tables=True, entries=ent, m=matched):
        k = np.array(kf, np.int32); o = np.array(off, np.int32)
        return L.sd_batch_search_by_projection_sim3(b.h, n_jobs, fc._p(k) if tables else None, fc._p(S) if tables else None,
                                                    fc._p(o) if tables else None, C.c_void_p(entries.data_ptr()), C.c_void_p(pts.data_ptr()),
                                                    C.c_void_p(desc.data_ptr()), 5, C.c_void_p(m.data_ptr()) if m is not None else None, fc._p(cam), th,
                                                    C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), None)

    def bowkf(n=1, k1=(0,), k2=(1,)):
        a = np.array(k1, np.int32); d = np.array(k2, np.int32)
        return L.sd_batch_search_by_bow_kf(b.h, n, fc._p(a), fc._p(d), None, None, C.c_float(0.75), 1, None)

    for call in (fuse, proj):
        assert call() == fe.SD_OK
        assert call(off=(1, 5)) == fe.SD_ERR_INVALID and call(off=(0, -2)) == fe.SD_ERR_INVALID
        assert call(n_jobs=2, kf=(0, 0), off=(0, 4, 2)) == fe.SD_ERR_INVALID
        assert call(th=0) == fe.SD_ERR_INVALID and call(th=-1) == fe.SD_ERR_INVALID
        assert call(tables=False) == fe.SD_ERR_INVALID
        assert call(kf=(SLOTS,)) == fe.SD_ERR_INVALID and call(kf=(-1,)) == fe.SD_ERR_INVALID
        assert call(n_jobs=-1) == fe.SD_ERR_INVALID and call(n_jobs=0) == fe.SD_OK
    assert proj(m=None) == fe.SD_ERR_INVALID
    assert bowkf() == fe.SD_OK and bowkf(n=SLOTS + 1, k1=(0,) * (SLOTS + 1), k2=(1,) * (SLOTS + 1)) == fe.SD_ERR_INVALID
    assert bowkf(k1=(SLOTS,)) == fe.SD_ERR_INVALID and bowkf(k2=(-1,)) == fe.SD_ERR_INVALID and bowkf(n=0) == fe.SD_OK
    # an index outside its table is found on the device: read as -1, reported by the downloads of that call only
    bad = torch.from_numpy(np.array([0, 1, 5, 2, -2], np.int32)).cuda()
    best = np.zeros((5, 2), np.int32); hits = np.zeros(5, fc.HIT_DTYPE); assigned = np.zeros(ws.cap, np.int32); ne, nf = C.c_int(), C.c_int()
    assert fuse(entries=bad) == fe.SD_OK
    assert L.sd_batch_download_fuse(b.h, 0, fc._p(best), fc._p(hits), 5, C.byref(ne), C.byref(nf)) == fe.SD_ERR_INVALID
    assert fuse() == fe.SD_OK
    assert L.sd_batch_download_fuse(b.h, 0, fc._p(best), fc._p(hits), 5, C.byref(ne), C.byref(nf)) == fe.SD_OK and ne.value == 5
    dl = lambda job=0, cap=ws.cap, ce=5: L.sd_batch_download_projection_sim3(b.h, job, fc._p(assigned), cap, fc._p(best), ce, C.byref(ne), C.byref(nf))
    assert proj(entries=bad) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
    assert proj() == fe.SD_OK and dl() == fe.SD_OK and ne.value == 5
    badm = matched.clone(); badm[0, 0] = 5
    assert proj(m=badm) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
    badm[0, 0] = -3
    assert proj(m=badm) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
    assert proj() == fe.SD_OK and dl() == fe.SD_OK
    assert dl(job=1) == fe.SD_ERR_INVALID and dl(ce=4) == fe.SD_ERR_CAPACITY and dl(cap=ws.cap - 1) == fe.SD_ERR_CAPACITY
    assert L.sd_batch_download_projection_sim3(b.h, 0, fc._p(assigned), ws.cap, None, 0, C.byref(ne), C.byref(nf)) == fe.SD_OK and ne.value == 5
    assert L.sd_batch_download_projection_sim3(b.h, 0, None, 0, None, 0, C.byref(ne), C.byref(nf)) == fe.SD_OK      # only the counts
    # a slot whose grid is stale: extraction invalidates it
    ws.b.extract_host(np.full((2, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws.b.sync()
    assert fuse() == fe.SD_ERR_STATE and proj() == fe.SD_ERR_STATE
    ws.b.extract_host(np.full((SLOTS, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws.b.sync()
    # slots on which sd_batch_compute_bow has never run
    w2 = tc.Workspace(fe, 2, tc.vocabulary(synth, 5))
    try:
        a = np.array([0], np.int32); d = np.array([1], np.int32)
        assert L.sd_batch_search_by_bow_kf(w2.b.h, 1, fc._p(a), fc._p(d), None, None, C.c_float(0.75), 1, None) == fe.SD_ERR_STATE
    finally:
        w2.close()
