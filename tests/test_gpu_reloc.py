"""GPU parity of sd_batch_search_by_projection_reloc with the sequential CPU oracle (tests/cpp/reloc_oracle.cpp): every crafted case of
reloc_cases.py, the 1-ulp scans, the shapes at which the kernels take another path, seeded random scenes, the independence of a job
from its launch, and the refusals -- frame_point, from_kf, exits, best pairs and nmatches byte for byte."""
import ctypes as C

import numpy as np
import pytest

import fuse_cases as fc
import reloc_cases as rc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SLOTS = 8


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = rc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    assert w.cap >= rc.SCAN_STEPS
    yield w
    w.close()


def check(ws, scene, cam=rc.CAM, upload=True):
    want, _ = rc.cpu_search(scene, cam=cam, lv=ws.lv)
    rc.assert_same(scene, rc.device_search(ws, scene, cam=cam, upload=upload), want)
    return want


def test_crafted_cases(ws):
    sc = rc.crafted_scene()
    want = check(ws, sc)
    rc.check_expect(sc, want)


def test_v_on_the_lower_image_bound(ws):
    sc = rc.v_min_scene()
    rc.check_expect(sc, check(ws, sc, cam=rc.CAM_VMIN))


def test_nan_and_infinite_projections(ws):
    sc = rc.nan_scene()
    rc.check_expect(sc, check(ws, sc))


@pytest.mark.parametrize("kind", rc.SCAN_KINDS)
def test_threshold_scans(ws, kind):
    sc = rc.scan_scene(kind)
    want = check(ws, sc, cam=sc["cam"])
    reached = np.isin(want[0][2], (rc.X["matched"], rc.X["no_free"]))
    assert 0 < int(reached.sum()) < rc.SCAN_STEPS


@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(ws, seed):
    """3 jobs (th 10 / ORBdist 100 and th 3 / ORBdist 64) x 260 keyframe features over one frame of about 390 features."""
    want = check(ws, rc.random_scene(seed))
    assert sum(w[4] for w in want) > 60


@pytest.mark.parametrize("n_kf,n_frame", [(0, None), (1, None), (63, None), (64, None), (65, None), (129, None), (5, 0)])
def test_sizes(ws, n_kf, n_frame):
    """0 / 1 / 63 / 64 / 65 / 129 keyframe features (the replay works in chunks of 64), and a frame without features."""
    (fp, frm, ex, best, nm), = check(ws, rc.sized_scene(n_kf, n_frame))
    if n_frame == 0:
        assert nm == 0 and list(ex) == [rc.X["window_empty"]] * n_kf
    else:
        assert nm >= n_kf // 2


def test_window_of_64_free_members_is_answered(ws):
    """66 identical points on 64 free members: takers 65 and 66 find every key taken and the window held no more -> no_free."""
    (fp, frm, ex, best, nm), = check(ws, rc.dense_window_scene(64, 66))
    assert nm == 64 and list(ex[64:66]) == [rc.X["no_free"]] * 2


def test_list_bound_is_reported_not_guessed(ws, fe):
    """70 free members within ORBdist of 66 identical points: the 65th finds its 64 kept keys taken while the window held 70.  The
    oracle has an answer; the library refuses the call's results, the twin with 64 takers is answered, and the next call is clean."""
    sc = rc.dense_window_scene(70, 66)
    want, _ = rc.cpu_search(sc, lv=ws.lv)
    assert want[0][4] == 66
    with pytest.raises(fe.SdError) as e:
        rc.device_search(ws, sc)
    assert e.value.code == fe.SD_ERR_UNSUPPORTED
    (fp, frm, ex, best, nm), = check(ws, rc.dense_window_scene(70, 64))
    assert nm == 64


def test_chain_of_65(ws):
    """Every keyframe feature is displaced by the one before it: a round of the replay commits one feature, over the chunk of 64."""
    sc = rc.chain_scene()
    (fp, frm, ex, best, nm), = check(ws, sc)
    assert nm == 65 and list(frm[:65]) == sc["want_chain"]


def _jobs_scene():
    sc = rc.random_scene(3)
    return sc, rc.cpu_search(sc)[0]


def test_a_job_does_not_depend_on_its_launch(ws):
    """1 / 2 / 65 jobs sharing the frame slot, permuted and repeated: each gives the bytes it gives alone, and a second run the same."""
    sc, want = _jobs_scene()
    ws.upload_grid(sc["kfs"])
    alone = [rc.device_search(ws, sc, upload=False, jobs=[j])[0] for j in sc["jobs"]]
    rc.assert_same(sc, alone, want, "alone")
    for order in ([1, 0], [2, 1, 0], [1, 1, 0, 2, 2, 0], [q % 3 for q in range(65)]):
        jobs = [sc["jobs"][q] for q in order]
        got = rc.device_search(ws, sc, upload=False, jobs=jobs)
        rc.assert_same(sc, got, [want[q] for q in order], "order %r" % (order[:6],))
        again = rc.device_search(ws, sc, upload=False, jobs=jobs)
        for a, b in zip(got, again):
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def test_the_call_does_not_wait_for_the_stream(ws):
    """Behind a long queue of work on the caller's stream the call returns while the stream is still busy."""
    import torch
    sc, want = _jobs_scene()
    ws.upload_grid(sc["kfs"])
    rc.device_search(ws, sc, upload=False)                        # the library-owned tables have grown
    st = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    a = a @ a * 1e-3                                               # the first product loads its kernels
    torch.cuda.synchronize()
    n = len(sc["jobs"])
    kfp = np.full((n, ws.cap), -1, np.int32); fp = np.full((n, ws.cap), -1, np.int32)
    for q, j in enumerate(sc["jobs"]):
        kfp[q, :len(j["kf_point"])] = j["kf_point"]; fp[q, :len(j["frame_point"])] = j["frame_point"]
    d_kfp, d_fp = torch.from_numpy(kfp).cuda(), torch.from_numpy(fp).cuda()
    d_pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda(); d_desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
    T = np.array([np.asarray(j["Tcw"], np.float32).reshape(16) for j in sc["jobs"]])
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(60):
            a = a @ a * 1e-3
        ws.b.search_by_projection_reloc([0] * n, [j["kf"] for j in sc["jobs"]], T, [j["th"] for j in sc["jobs"]], [j["orb"] for j in sc["jobs"]],
                                        d_kfp.data_ptr(), d_fp.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), rc.CAM, n_points=len(sc["points"]),
                                        stream=st.cuda_stream)
        busy = not st.query()
    st.synchronize()
    assert busy, "the stream had drained when the call returned"
    got = [ws.b.download_reloc_matches(q) for q in range(n)]
    # found flags are not passed here: compare with an oracle run without them
    sc2 = dict(sc); sc2["jobs"] = [dict(j, found=None) for j in sc["jobs"]]
    rc.assert_same(sc2, got, rc.cpu_search(sc2, lv=ws.lv)[0], "behind a busy stream")


def test_refusals(ws, fe):
    import torch
    sc = rc.sized_scene(5)
    ws.upload_grid(sc["kfs"])
    L, b = fe.lib(), ws.b
    cam = fe.camera_array(tc.CAM)
    npts = len(sc["points"])
    pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda()
    desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
    job = sc["jobs"][0]
    kfp0 = np.full((2, ws.cap), -1, np.int32); kfp0[0, :5] = job["kf_point"]; kfp0[1, :5] = job["kf_point"]
    kfp = torch.from_numpy(kfp0).cuda(); fpt = torch.full((2, ws.cap), -1, dtype=torch.int32).cuda()
    T = np.tile(np.asarray(job["Tcw"], np.float32).reshape(16), 2)
    out = [C.c_void_p(), C.c_void_p(), C.c_void_p()]

    def call(n_jobs=1, frame=(0, 0), kf=(1, 1), th=(10.0, 10.0), orb=(100, 100), tables=True, k=kfp, f=fpt, points=True):
        fi = np.array(frame, np.int32); ki = np.array(kf, np.int32); t = np.array(th, np.float32); o = np.array(orb, np.int32)
        return L.sd_batch_search_by_projection_reloc(b.h, n_jobs, fc._p(fi) if tables else None, fc._p(ki), fc._p(T), fc._p(t), fc._p(o),
                                                     C.c_void_p(k.data_ptr()) if k is not None else None, C.c_void_p(f.data_ptr()) if f is not None else None,
                                                     None, C.c_void_p(pts.data_ptr()) if points else None, C.c_void_p(desc.data_ptr()), npts, fc._p(cam),
                                                     C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), None)

    rows = [np.zeros(ws.cap, np.int32) for _ in range(3)] + [np.zeros((ws.cap, 2), np.int32)]
    nm = C.c_int()
    dl = lambda job=0, cap=ws.cap: L.sd_batch_download_reloc_matches(b.h, job, fc._p(rows[0]), fc._p(rows[1]), fc._p(rows[2]), fc._p(rows[3]), cap, C.byref(nm))
    assert call() == fe.SD_OK and dl() == fe.SD_OK and nm.value >= 3
    assert call(n_jobs=2) == fe.SD_OK and dl(1) == fe.SD_OK and dl(2) == fe.SD_ERR_INVALID and dl(-1) == fe.SD_ERR_INVALID
    assert dl(cap=ws.cap - 1) == fe.SD_ERR_CAPACITY
    assert L.sd_batch_download_reloc_matches(b.h, 0, None, None, None, None, 0, C.byref(nm)) == fe.SD_OK      # only the count
    # ORBdist > 255 would index with bestIdx2 == -1 in the reference; th <= 0
    assert call(orb=(256, 100)) == fe.SD_ERR_INVALID and call(orb=(-1, 100)) == fe.SD_ERR_INVALID and call(orb=(255, 100)) == fe.SD_OK
    assert call(n_jobs=2, orb=(100, 256)) == fe.SD_ERR_INVALID
    assert call(th=(0.0, 10.0)) == fe.SD_ERR_INVALID and call(th=(-1.0, 10.0)) == fe.SD_ERR_INVALID and call(th=(float("nan"), 10.0)) == fe.SD_ERR_INVALID
    # caps and tables
    assert call(n_jobs=-1) == fe.SD_ERR_INVALID and call(n_jobs=0) == fe.SD_OK and call(tables=False) == fe.SD_ERR_INVALID
    assert call(n_jobs=fe.SD_RELOC_MAX_JOBS + 1) == fe.SD_ERR_INVALID
    assert call(frame=(SLOTS, 0)) == fe.SD_ERR_INVALID and call(kf=(-1, 1)) == fe.SD_ERR_INVALID
    assert call(k=None) == fe.SD_ERR_INVALID and call(f=None) == fe.SD_ERR_INVALID and call(points=False) == fe.SD_ERR_INVALID
    assert dl() == fe.SD_ERR_INVALID                              # a refused call leaves no job to download
    # an index outside its table is found on the device: read as -1, reported by the downloads of that call only
    for bad in (npts, -2):
        kb = kfp.clone(); kb[0, 2] = bad
        assert call(k=kb) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
        fb = fpt.clone(); fb[0, 4] = bad
        assert call(f=fb) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
    assert call() == fe.SD_OK and dl() == fe.SD_OK
    # a slot whose grid is stale: extraction invalidates it (the frame's, then the keyframe's)
    ws.b.extract_host(np.full((1, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws.b.sync()
    assert call() == fe.SD_ERR_STATE and call(frame=(1, 1)) == fe.SD_OK and call(kf=(0, 0)) == fe.SD_ERR_STATE
    ws.b.extract_host(np.full((SLOTS, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws.b.sync()


# ---------------------------------------------------------------- the cascade: sd_batch_relocalize_refine
import pose_cases as pc  # noqa: E402

CASCADE_SLOTS = 2 * len(rc.CASCADE_CASES)


@pytest.fixture(scope="module")
def ws24(gpu, fe, synth):
    w = rc.Workspace(fe, CASCADE_SLOTS, tc.vocabulary(synth, 5))
    yield w
    w.close()


@pytest.fixture(scope="module")
def cascade(ws24):
    sc = rc.cascade_scene()
    return sc, rc.cpu_refine(sc, lv=ws24.lv)


def test_cascade_stage_by_stage(ws24, cascade):
    sc, want = cascade
    got = rc.device_refine(ws24, sc)
    rc.check_stages(ws24, sc, sc["jobs"], got)


def test_cascade_gates_free_running(ws24, cascade):
    """The crafted cases that put nGood on every gate: stage_reached, matched, n_good, n_additional (and with them the final assignment
    and the outlier flags) equal the free-running oracle's; the poses agree within pose_close."""
    sc, want = cascade
    got = rc.device_refine(ws24, sc)
    for name, expect, g, w in zip(sc["names"], sc["want"], got, want):
        n2 = len(w[1])
        d = (int(g[0]["stage_reached"]), int(g[0]["matched"]), tuple(int(x) for x in g[0]["n_good"]), tuple(int(x) for x in g[0]["n_additional"]))
        assert d == expect == rc.decisions(w)[:4], "%s: %r, oracle %r" % (name, d, rc.decisions(w)[:4])
        assert g[1][:n2].tobytes() == w[1].tobytes() and np.all(g[1][n2:] == -1), name + ": final assignment"
        assert g[2][:n2].tobytes() == w[2].tobytes() and np.all(g[2][n2:] == 0), name + ": mvbOutlier"
        for k in range(3):
            assert pc.pose_close(g[0]["Tcw_stage"][k], w[0]["Tcw_stage"][k]), "%s: pose after optimisation %d" % (name, k)


@pytest.mark.parametrize("seed", range(3))
def test_random_cascades_stage_by_stage(ws24, seed):
    sc = rc.random_cascade_scene(seed)
    got = rc.device_refine(ws24, sc)
    rc.check_stages(ws24, sc, sc["jobs"], got)


def test_a_cascade_does_not_depend_on_its_launch(ws24, cascade):
    """Jobs alone, permuted, repeated to 65 and run twice: every job gives the bits it gives in the full call."""
    sc, _ = cascade
    full = rc.device_refine(ws24, sc)
    same = lambda a, b: a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    n = len(sc["jobs"])
    for order in ([6], [10, 3], list(range(n))[::-1], [q % n for q in range(65)], [q % n for q in range(65)]):
        got = rc.device_refine(ws24, sc, upload=False, jobs=[sc["jobs"][q] for q in order])
        for g, q in zip(got, order):
            assert same(g, full[q]), "job %d in a call of %d" % (q, len(order))


def test_the_cascade_does_not_wait_for_the_stream(ws24, cascade):
    """No host synchronisation between the steps: behind a long queue on the caller's stream the whole cascade is enqueued and the call
    returns while the stream is still busy."""
    import torch
    sc, _ = cascade
    full = rc.device_refine(ws24, sc)                             # the tables have grown
    n = len(sc["jobs"])
    kfp = np.full((n, ws24.cap), -1, np.int32); fp = np.full((n, ws24.cap), -1, np.int32)
    for q, j in enumerate(sc["jobs"]):
        kfp[q, :len(j["kf_point"])] = j["kf_point"]; fp[q, :len(j["frame_point"])] = j["frame_point"]
    d_kfp, d_fp = torch.from_numpy(kfp).cuda(), torch.from_numpy(fp).cuda()
    d_pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda(); d_desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
    T = np.array([np.asarray(j["Tcw"], np.float32).reshape(16) for j in sc["jobs"]])
    st = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    a = a @ a * 1e-3
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(60):
            a = a @ a * 1e-3
        ws24.b.relocalize_refine([j["frame"] for j in sc["jobs"]], [j["kf"] for j in sc["jobs"]], T, d_kfp.data_ptr(), d_fp.data_ptr(), d_pts.data_ptr(),
                                 d_desc.data_ptr(), rc.CAM, n_points=len(sc["points"]), stream=st.cuda_stream)
        busy = not st.query()
    st.synchronize()
    assert busy, "the stream had drained when the call returned"
    for q in range(n):
        g = ws24.b.download_reloc(q)
        assert g[0].tobytes() == full[q][0].tobytes() and g[1].tobytes() == full[q][1].tobytes() and g[2].tobytes() == full[q][2].tobytes()


def test_cascade_refusals(ws24, fe, cascade):
    import torch
    sc, _ = cascade
    ws24.upload_grid(sc["kfs"])
    L, b, cap = fe.lib(), ws24.b, ws24.cap
    cam = fe.camera_array(tc.CAM)
    npts = len(sc["points"])
    pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda(); desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
    j = sc["jobs"][0]
    kfp0 = np.full((2, cap), -1, np.int32); fp0 = np.full((2, cap), -1, np.int32)
    kfp0[:, :len(j["kf_point"])] = j["kf_point"]; fp0[:, :len(j["frame_point"])] = j["frame_point"]
    kfp, fpt = torch.from_numpy(kfp0).cuda(), torch.from_numpy(fp0).cuda()
    T = np.tile(np.asarray(j["Tcw"], np.float32).reshape(16), 2)
    out = C.c_void_p()

    def call(n_jobs=1, frame=(0, 0), kf=(1, 1), tables=True, k=kfp, f=fpt, points=True):
        fi = np.array(frame, np.int32); ki = np.array(kf, np.int32)
        return L.sd_batch_relocalize_refine(b.h, n_jobs, fc._p(fi) if tables else None, fc._p(ki), fc._p(T), C.c_void_p(k.data_ptr()) if k is not None else None,
                                            C.c_void_p(f.data_ptr()) if f is not None else None, C.c_void_p(pts.data_ptr()) if points else None,
                                            C.c_void_p(desc.data_ptr()), npts, fc._p(cam), C.byref(out), None)

    res = np.zeros(1, fe.RELOC_RESULT_DTYPE); row = np.zeros(cap, np.int32); flags = np.zeros(cap, np.uint8)
    dl = lambda job=0, c=cap: L.sd_batch_download_reloc(b.h, job, fc._p(res), fc._p(row), fc._p(flags), c)
    assert call() == fe.SD_OK and dl() == fe.SD_OK and res[0]["n_good"][0] == 9
    assert call(n_jobs=2) == fe.SD_OK and dl(1) == fe.SD_OK and dl(2) == fe.SD_ERR_INVALID and dl(c=cap - 1) == fe.SD_ERR_CAPACITY
    assert call(n_jobs=-1) == fe.SD_ERR_INVALID and call(n_jobs=fe.SD_RELOC_MAX_JOBS + 1) == fe.SD_ERR_INVALID and call(tables=False) == fe.SD_ERR_INVALID
    assert call(frame=(CASCADE_SLOTS, 0)) == fe.SD_ERR_INVALID and call(kf=(-1, 1)) == fe.SD_ERR_INVALID
    assert call(k=None) == fe.SD_ERR_INVALID and call(f=None) == fe.SD_ERR_INVALID and call(points=False) == fe.SD_ERR_INVALID
    assert call(n_jobs=0) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
    for bad in (npts, -2):                                        # read as -1, reported by the downloads of that call only
        kb = kfp.clone(); kb[0, 1] = bad
        assert call(k=kb) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
        fb = fpt.clone(); fb[0, 3] = bad
        assert call(f=fb) == fe.SD_OK and dl() == fe.SD_ERR_INVALID
    assert call() == fe.SD_OK and dl() == fe.SD_OK
    ws24.b.extract_host(np.full((1, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws24.b.sync()
    assert call() == fe.SD_ERR_STATE
    ws24.b.extract_host(np.full((CASCADE_SLOTS, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws24.b.sync()
