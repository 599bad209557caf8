"""GPU parity of sd_batch_fuse / sd_distinctive_descriptors_device with the sequential CPU oracle (tests/cpp/fuse_oracle.cpp): every
crafted case of fuse_cases.py, the 1-ulp threshold scans, the job and window shapes at which the kernels take another path and a seeded
random sweep, all byte for byte -- (bestIdx, bestDist) per entry, the sd_fuse_hit records and the return values."""
import ctypes as C

import numpy as np
import pytest

import fuse_cases as fc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SLOTS = 12


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = fc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    assert fc.inv_sigma2(w.lv).tobytes() == w.ex.mvInvLevelSigma2.tobytes()
    yield w
    w.close()


def check(ws, scene):
    want, _ = fc.cpu_run(scene, lv=ws.lv)
    got = fc.device_run(ws, scene)
    fc.assert_same(scene, got, want)
    return want


def test_crafted_cases(ws):
    """All crafted cases in one call: four jobs over three keyframes (one without features), one job empty."""
    sc = fc.crafted_scene()
    want = check(ws, sc)
    fc.check_expectations(sc, want)


@pytest.mark.parametrize("kind", fc.SCAN_KINDS)
def test_threshold_scans(ws, kind):
    sc = fc.scan_scene(kind)
    (best, hits, nf), = check(ws, sc)
    assert 0 < nf < 512


@pytest.fixture(scope="module")
def shared_scene():
    return fc.random_scene(11, 3, 200, n_features=150)


@pytest.mark.parametrize("n_jobs", [1, 2, 17])
def test_jobs_per_call(ws, shared_scene, n_jobs):
    """1, 2 and 17 jobs over three slots that the jobs share; every job names the one candidate list."""
    sc = dict(shared_scene)
    base = shared_scene["jobs"]
    sc["jobs"] = [base[q % 3] for q in range(n_jobs)]
    want = check(ws, sc)
    assert sum(w[2] for w in want) > 0


def test_more_jobs_than_max_images(ws, shared_scene):
    sc = dict(shared_scene)
    sc["jobs"] = [shared_scene["jobs"][q % 3] for q in range(SLOTS + 5)]
    check(ws, sc)


def test_job_sizes(ws):
    """Jobs of 0, 1, 63, 64, 65 and 257 entries in one call."""
    sc = fc.sized_jobs_scene()
    want = check(ws, sc)
    assert [len(w[0]) for w in want] == [0, 1, 63, 64, 65, 257]


@pytest.mark.parametrize("n", [65, 130])
def test_window_of_more_than_64_features(ws, n):
    sc = fc.dense_window_scene(n)
    want = check(ws, sc)
    assert np.all(want[0][0][:, 1] == 12)


def test_all_hits_contend_for_one_feature(ws):
    sc = fc.contention_scene(40)
    (best, hits, nf), = check(ws, sc)
    assert nf == 40 and int((hits["action"] == fc.ADD).sum()) == 1 and int((hits["action"] == fc.MEET_CANDIDATE).sum()) == 39
    assert np.all(hits["other"][1:] == 0)


def test_keyframe_filled_to_capacity(ws):
    sc = fc.full_keyframe_scene(ws.cap)
    assert len(sc["kfs"][0]["kp"]) == ws.cap
    (best, hits, nf), = check(ws, sc)
    assert nf > 10


def test_scratch_grows_with_a_larger_second_call(gpu, fe, synth):
    """A fresh workspace: a call of 3 entries, then one of 17 jobs and thousands of entries."""
    w = fc.Workspace(fe, 3, tc.vocabulary(synth, 5))
    try:
        small = fc.contention_scene(3)
        fc.assert_same(small, fc.device_run(w, small), fc.cpu_run(small, lv=w.lv)[0])
        big = fc.random_scene(12, 3, 250, n_features=150)
        big["jobs"] = [big["jobs"][q % 3] for q in range(17)]
        fc.assert_same(big, fc.device_run(w, big), fc.cpu_run(big, lv=w.lv)[0])
        fc.assert_same(small, fc.device_run(w, small), fc.cpu_run(small, lv=w.lv)[0])
    finally:
        w.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_sweep(ws, seed):
    """6 scenes x 8 targets x 300 points, stereo and mono mixed, random feature states, a few -1 entries."""
    sc = fc.random_scene(seed, 8, 300, n_features=220, shared_list=seed % 2 == 0)
    want = check(ws, sc)
    assert sum(w[2] for w in want) > 100


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_proposals_plus_the_models_tail_equal_the_literal_fuse(ws, seed):
    """The single-job reformulation test of test_fuse_oracle.py with the device as the searcher."""
    sc = fc.model_scene(seed)
    lit, ref = fc.build_model(sc), fc.build_model(sc)
    try:
        n1 = lit.fuse(0, sc["cand"])
        entries, state = ref.snapshot(0, sc["cand"])
        rec, desc, _, _ = ref.points()
        job = dict(name=sc["name"], kfs=sc["kfs"], points=rec, pdesc=desc, jobs=[(0, entries, state)], th=3.0)
        (best, hits, nf), = fc.device_run(ws, job)
        n2 = ref.tail(0, sc["cand"], best)
        assert n1 == n2 == nf
        assert lit.dump() == ref.dump()
        assert set(np.unique(hits["action"])) == {fc.ADD, fc.MEET_KF, fc.MEET_BAD, fc.MEET_CANDIDATE}
    finally:
        lit.close(); ref.close()


def test_invalid_arguments(ws, fe):
    import torch
    sc = fc.contention_scene(5)
    fc.device_run(ws, sc)
    L, b = fe.lib(), ws.b
    cam = fe.camera_array(tc.CAM)
    pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda()
    desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
    ent = torch.from_numpy(sc["jobs"][0][1].copy()).cuda()
    T = np.ascontiguousarray(sc["kfs"][0]["Tcw"], np.float32).reshape(16)
    out = [C.c_void_p(), C.c_void_p(), C.c_void_p()]

    def call(n_jobs=1, kf=(0,), off=(0, 5), th=3.0, tables=True, n_points=5, entries=ent):
        k = np.array(kf, np.int32); o = np.array(off, np.int32)
        return L.sd_batch_fuse(b.h, n_jobs, fc._p(k) if tables else None, fc._p(T) if tables else None, fc._p(o) if tables else None,
                               C.c_void_p(entries.data_ptr()), C.c_void_p(pts.data_ptr()), C.c_void_p(desc.data_ptr()), n_points, None,
                               fc._p(cam), C.c_float(th), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), None)

    assert call() == fe.SD_OK
    assert call(off=(1, 5)) == fe.SD_ERR_INVALID                       # cand_offset[0] != 0
    assert call(off=(0, -2)) == fe.SD_ERR_INVALID                      # descending
    assert call(n_jobs=2, kf=(0, 0), off=(0, 4, 2)) == fe.SD_ERR_INVALID
    assert call(th=0.0) == fe.SD_ERR_INVALID and call(th=-1.0) == fe.SD_ERR_INVALID
    assert call(tables=False) == fe.SD_ERR_INVALID                     # n_jobs > 0 with NULL tables
    assert call(kf=(SLOTS,)) == fe.SD_ERR_INVALID and call(kf=(-1,)) == fe.SD_ERR_INVALID
    assert call(n_jobs=-1) == fe.SD_ERR_INVALID
    assert call(n_jobs=0) == fe.SD_OK
    # a point index out of range is found on the device: searched as -1, reported by the download
    bad = torch.from_numpy(np.array([0, 1, 5, 2, -2], np.int32)).cuda()
    assert call(entries=bad) == fe.SD_OK
    best = np.zeros((5, 2), np.int32); hits = np.zeros(5, fc.HIT_DTYPE); ne, nf = C.c_int(), C.c_int()
    assert L.sd_batch_download_fuse(b.h, 0, fc._p(best), fc._p(hits), 5, C.byref(ne), C.byref(nf)) == fe.SD_ERR_INVALID
    assert call() == fe.SD_OK                                          # never fatal: the next call is clean
    assert L.sd_batch_download_fuse(b.h, 0, fc._p(best), fc._p(hits), 5, C.byref(ne), C.byref(nf)) == fe.SD_OK and ne.value == 5
    assert L.sd_batch_download_fuse(b.h, 1, fc._p(best), fc._p(hits), 5, C.byref(ne), C.byref(nf)) == fe.SD_ERR_INVALID
    assert L.sd_batch_download_fuse(b.h, 0, fc._p(best), fc._p(hits), 4, C.byref(ne), C.byref(nf)) == fe.SD_ERR_CAPACITY
    # a slot whose grid is stale: extraction invalidates it
    ws.b.extract_host(np.full((1, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws.b.sync()
    assert call() == fe.SD_ERR_STATE
    ws.b.extract_host(np.full((SLOTS, tc.GEOM["H"], tc.GEOM["W"]), 128, np.uint8)); ws.b.sync()


# ---------------------------------------------------------------- ComputeDistinctiveDescriptors
def run_distinctive(fe, lists):
    import torch
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    flat = np.concatenate([np.asarray(x, np.uint8).reshape(-1, 32) for x in lists] + [np.zeros((1, 32), np.uint8)])
    d = torch.from_numpy(flat.reshape(-1).copy()).cuda()
    best = torch.full((len(lists),), -7, dtype=torch.int32).cuda()
    out = torch.full((len(lists), 32), 0xAB, dtype=torch.uint8).cuda()
    keep = fe.distinctive_descriptors(off, d.data_ptr(), best.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    del keep
    return best.cpu().numpy(), out.cpu().numpy()


def test_distinctive_descriptors(gpu, fe):
    """The CPU cases (N = 0, 1, 2, 3, even N with tied medians), N = 64, 65 and 200, and 1,000 random points in one call."""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = fc.flipped(a, 10, rng)
    e = fc.flipped(a, 100, rng); f = fc.flipped(e, 4, rng); g = fc.flipped(a, 6, rng)
    lists = [np.zeros((0, 32), np.uint8), a[None], np.stack([a, fc.flipped(a, 40, rng)]), np.stack([a, b, fc.flipped(b, 12, rng)]),
             np.stack([a, b, a, b]), np.stack([e, f, a, g]), np.stack([a, g, e, f])]
    for n in (64, 65, 200):
        c = rng.integers(0, 256, 32, dtype=np.uint8)
        lists.append(np.stack([fc.flipped(c, int(rng.integers(0, 90)), rng) for _ in range(n)]))
    for _ in range(1000):
        n = int(rng.integers(0, 40))
        c = rng.integers(0, 256, 32, dtype=np.uint8)
        lists.append(np.stack([fc.flipped(c, int(rng.integers(0, 60)), rng) for _ in range(n)]) if n else np.zeros((0, 32), np.uint8))
    best, out = run_distinctive(fe, lists)
    for p, d in enumerate(lists):
        w, wd = fc.distinctive(d)
        assert best[p] == w, "point %d (N = %d): BestIdx %d vs %d" % (p, len(d), best[p], w)
        assert out[p].tobytes() == (wd.tobytes() if w >= 0 else bytes([0xAB]) * 32), "point %d: descriptor" % p
    assert best[0] == -1 and best[4] == 0 and best[5] == 0 and best[6] == 2
