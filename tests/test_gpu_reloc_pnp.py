"""The relocalisation chain sd_batch_relocalize_pnp (Tracking.cc:2256-2358 as one launch sequence) stage by stage, in the manner of
tests/test_gpu_reloc.py, each stage from the device's own input: the gathered problem byte for byte against numpy, the PnP record bit for
bit against the CPU oracle on the device's own problem, the row handed over (lines 2300-2309), and the cascade byte for byte against the
existing sd_batch_relocalize_refine fed the device's pose and row through the host.  Jobs: the twelve cascade cases of
tests/reloc_cases.py (their BoW rows: 9 .. 50 exact matches plus 2 - 3 wrong ones), one of them cut to 0 / 14 / 15 matches, a match on
a bad point, and a job of kind 0 beside a matched one on the same frame slot."""
import numpy as np
import pytest

import pnp_cases as pc
import reloc_cases as rc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SOURCE = "2321_ngood_49"                 # 49 exact matches + 2 wrong ones: the row the cut jobs are made from
# The cascade scenes put their first 20 anchors on ONE image row (v = 25), i.e. in a plane through the camera centre: a job with up to
# about 22 matches is a degenerate PnP problem, whose kind is whatever the oracle says (kinds 0 and 2 occur).  These four are not:
POSED = ("2321_ngood_49", "2321_ngood_50", "matches_14", "matches_15")


def _cut(job, keep):
    q = dict(job)
    fp = job["frame_point"].copy()
    idx = np.nonzero(fp >= 0)[0]
    kept = idx[:49:3][:keep]                 # spread over the scene's three rows of anchors: one row alone lies in a plane through the camera centre
    fp[np.setdiff1d(idx, kept)] = -1
    q["frame_point"] = fp
    return q


def _expected_corr(sc, pts, lv, job, row):
    """The PnPsolver constructor's gather (PnPsolver.cc:79-101) in numpy."""
    kp = np.ascontiguousarray(sc["kfs"][job["frame"]]["kp"], tc.KP_DTYPE)
    row = row[:len(kp)]
    keep = np.nonzero((row >= 0) & ((pts["flags"][np.maximum(row, 0)] & 1) != 0))[0]
    want = np.zeros(len(keep), pc.CORR_DTYPE)
    want["xw"] = pts["xw"][row[keep]]; want["uv"] = np.stack([kp["x"][keep], kp["y"][keep]], 1)
    want["sigma2"] = lv.sigma2[kp["octave"][keep]]; want["tag"] = keep
    return want


@pytest.fixture(scope="module")
def chain(gpu, fe, synth):
    import torch
    ws = rc.Workspace(fe, 2 * len(rc.CASCADE_CASES), tc.vocabulary(synth, 5))
    try:
        sc = rc.cascade_scene()
        src = sc["jobs"][sc["names"].index(SOURCE)]
        jobs = list(sc["jobs"]) + [_cut(src, 0), _cut(src, 14), _cut(src, 15)]
        names = list(sc["names"]) + ["matches_0", "matches_14", "matches_15"]
        pts = np.ascontiguousarray(sc["points"], rc.MP_DTYPE).copy()
        bad_job = sc["names"].index("2325_sum_50")
        bad_i = int(np.nonzero(jobs[bad_job]["frame_point"] >= 0)[0][3])
        pts["flags"][jobs[bad_job]["frame_point"][bad_i]] &= ~np.uint32(1)                 # isBad(): the gather skips it (PnP:85)
        ws.upload_grid(sc["kfs"], rc.CAM)
        n = len(jobs)
        kfp = np.full((n, ws.cap), -1, np.int32); bow = np.full((n, ws.cap), -1, np.int32)
        for q, j in enumerate(jobs):
            kfp[q, :len(j["kf_point"])] = j["kf_point"]; bow[q, :len(j["frame_point"])] = j["frame_point"]
        d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda()
        d_desc = torch.from_numpy(np.ascontiguousarray(sc["pdesc"], np.uint8).reshape(-1).copy()).cuda()
        d_kfp, d_bow = torch.from_numpy(kfp).cuda(), torch.from_numpy(bow).cuda()
        probs = np.zeros(n, pc.PROBLEM_DTYPE)
        probs["K"] = [rc.CAM["fx"], rc.CAM["fy"], rc.CAM["cx"], rc.CAM["cy"]]; probs["n_iterations"] = 5
        for q, j in enumerate(jobs):          # as the crafted PnP cases: the first sampler seed under which the oracle keeps the job's decision
            corr = _expected_corr(sc, pts, ws.lv, j, bow[q])      # under both summation orders and both contraction settings (CPU only)
            for seed in range(1000 + 100 * q, 1100 + 100 * q):
                probs["seed"][q] = seed
                pr = dict(corr=corr, prob=probs[q:q + 1], **pc.DEFAULTS)
                if pc.stable(pr) and (names[q] not in POSED or pc.iterate(pr)[0]["kind"] == 1):      # and, where the geometry allows, a refined pose
                    break
            else:
                raise AssertionError("no stable seed for job %d" % q)
        fr, kf = [j["frame"] for j in jobs], [j["kf"] for j in jobs]
        ws.b.relocalize_pnp(fr, kf, probs, d_bow.data_ptr(), d_kfp.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), rc.CAM, n_points=len(pts), **pc.DEFAULTS)
        got = [ws.b.download_reloc_pnp(q) for q in range(n)]
        # the existing entry, fed the device's pose and row through the host
        d_row = torch.from_numpy(np.stack([g["row"] for g in got])).cuda()
        T = np.stack([g["pnp"]["Tcw"] for g in got]).astype(np.float32)
        ws.b.relocalize_refine(fr, kf, T, d_kfp.data_ptr(), d_row.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), rc.CAM, n_points=len(pts))
        ref = [ws.b.download_reloc(q) for q in range(n)]
        # and the chain once more with the batch reversed
        rev = list(range(n))[::-1]
        d_kfp2, d_bow2 = torch.from_numpy(kfp[rev].copy()).cuda(), torch.from_numpy(bow[rev].copy()).cuda()
        ws.b.relocalize_pnp([fr[q] for q in rev], [kf[q] for q in rev], probs[rev], d_bow2.data_ptr(), d_kfp2.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(),
                            rc.CAM, n_points=len(pts), **pc.DEFAULTS)
        got_rev = [ws.b.download_reloc_pnp(q) for q in range(n)][::-1]
        yield dict(ws=ws, sc=sc, jobs=jobs, names=names, pts=pts, bow=bow, probs=probs, got=got, ref=ref, rev=got_rev, bad=(bad_job, bad_i),
                   slots=(fr, kf), dev=dict(pts=d_pts, desc=d_desc, kfp=d_kfp, bow=d_bow))
    finally:
        ws.close()


def test_gathered_problem_byte_for_byte(chain):
    lv = chain["ws"].lv
    for q, (job, g) in enumerate(zip(chain["jobs"], chain["got"])):
        want = _expected_corr(chain["sc"], chain["pts"], lv, job, chain["bow"][q])
        assert g["corr"].tobytes() == want.tobytes(), chain["names"][q]
    bad_job, bad_i = chain["bad"]
    assert bad_i not in chain["got"][bad_job]["corr"]["tag"] and chain["bow"][bad_job][bad_i] >= 0
    sizes = {chain["names"][q]: len(g["corr"]) for q, g in enumerate(chain["got"])}
    assert all(chain["got"][chain["names"].index(k)]["inliers"].all() for k in ("matches_14", "matches_15"))
    assert (sizes["matches_0"], sizes["matches_14"], sizes["matches_15"], sizes[SOURCE]) == (0, 14, 15, 51)


def test_pnp_record_against_the_oracle_on_the_devices_own_problem(chain):
    kinds, held = set(), 0
    for q, g in enumerate(chain["got"]):
        pr = dict(corr=g["corr"], prob=chain["probs"][q:q + 1], **pc.DEFAULTS)
        ro, io, _ = pc.iterate(pr, order=1)
        assert pc.same_result(g["pnp"], ro) and g["inliers"].tobytes() == io.tobytes(), chain["names"][q]
        # and the sequential order's decisions: every job's seed was chosen so that the oracle keeps them under both orders and both
        # contraction settings (the fixture), so none is skipped
        assert pc.stable(pr), chain["names"][q]
        rs, is_, _ = pc.iterate(pr, order=0)
        assert (g["pnp"]["kind"], g["pnp"]["iteration"], g["pnp"]["n_inliers"]) == (rs["kind"], rs["iteration"], rs["n_inliers"]) and g["inliers"].tobytes() == is_.tobytes()
        held += 1
        kinds.add(int(g["pnp"]["kind"]))
    assert held == len(chain["got"])
    by = dict(zip(chain["names"], chain["got"]))
    assert by["matches_0"]["pnp"]["kind"] == 0 and by["2313_ngood_9"]["pnp"]["kind"] == 0           # N = 0; 9 inliers of 12 < min_inliers = 10
    assert all(by[k]["pnp"]["kind"] == 1 for k in POSED)
    assert by[SOURCE]["pnp"]["n_inliers"] == 49 and by["matches_14"]["pnp"]["n_inliers"] == 14 and by["matches_15"]["pnp"]["n_inliers"] == 15
    assert kinds == {0, 1, 2}
    T = by[SOURCE]["pnp"]["Tcw"].reshape(4, 4)                       # the scene's true pose is the identity
    assert np.abs(T - np.eye(4)).max() < 1e-3


def test_row_handed_over(chain):
    for q, g in enumerate(chain["got"]):
        want = np.full(chain["ws"].cap, -1, np.int32)
        tags = g["corr"]["tag"][g["inliers"] != 0]
        want[tags] = chain["bow"][q][tags]
        assert g["row"].tobytes() == want.tobytes(), chain["names"][q]
        if g["pnp"]["kind"] == 0:
            assert (g["row"] == -1).all()


def test_cascade_equals_relocalize_refine_fed_the_device_pose(chain):
    for q, (g, (res, fp, out)) in enumerate(zip(chain["got"], chain["ref"])):
        assert g["result"].tobytes() == res.tobytes() and g["frame_point"].tobytes() == fp.tobytes() and g["outlier"].tobytes() == out.tobytes(), chain["names"][q]
    by = dict(zip(chain["names"], chain["got"]))
    assert by[SOURCE]["result"]["n_good"][0] == 49 and by[SOURCE]["result"]["matched"] == 1        # the cascade case's own outcome, from the device pose
    assert by["2321_ngood_50"]["result"]["n_good"][0] == 50


def test_kind_0_job_beside_a_matched_one_on_the_same_frame_slot(chain):
    by = dict(zip(chain["names"], zip(chain["jobs"], chain["got"])))
    (j0, g0), (j1, g1) = by["matches_0"], by[SOURCE]
    assert j0["frame"] == j1["frame"] and g0["pnp"]["kind"] == 0 and g1["result"]["matched"] == 1
    assert g0["result"]["matched"] == 0 and g0["result"]["n_good"][0] == 0 and (g0["frame_point"] == -1).all() and not g0["outlier"].any()
    assert not g0["pnp"]["Tcw"].any() and g0["pnp"]["no_more"] == 1


def test_a_jobs_bytes_do_not_depend_on_its_neighbours(chain):
    for q, (a, b) in enumerate(zip(chain["got"], chain["rev"])):
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (chain["names"][q], k)


def test_refusals(chain, fe):
    ws, n = chain["ws"], 1
    probs = chain["probs"][:1].copy()

    def code(**kw):
        with pytest.raises(fe.SdError) as e:
            ws.b.relocalize_pnp([0], [1], kw.pop("problems", probs), 1, 1, 1, 1, rc.CAM, n_points=1, **dict(pc.DEFAULTS, **kw))
        return e.value.code

    assert code(min_set=5) == fe.SD_ERR_INVALID and code(epsilon=0.0) == fe.SD_ERR_INVALID and code(th2=0.0) == fe.SD_ERR_INVALID
    assert code(probability=1.0) == fe.SD_ERR_INVALID and code(max_iterations=pc.MAX_ITS + 1) == fe.SD_ERR_INVALID
    late = probs.copy(); late["start_iteration"] = pc.MAX_ITS
    assert code(problems=late) == fe.SD_ERR_INVALID
    with pytest.raises(fe.SdError):
        ws.b.relocalize_pnp([0], [1], probs, 0, 1, 1, 1, rc.CAM, n_points=1, **pc.DEFAULTS)                  # no BoW row


def test_ransac_and_the_chain_share_one_workspace_across_streams(chain, fe):
    """sd_pnp_ransac_device on one side stream, the chain on another, the same sd_pnp_ransac_device call again on the first: the PnP
    workspace of the device serves all three with no synchronisation until the end, and each gives what it gives alone."""
    import ctypes as C
    import torch
    ws, got, D = chain["ws"], chain["got"], pc.DEFAULTS
    prs = [dict(corr=g["corr"], prob=chain["probs"][q:q + 1]) for q, g in enumerate(got)]      # the chain's own gathered problems
    off, corr, probs = pc.pack(prs)
    want_res, want_inl = fe.pnp_ransac(off, corr, probs, **D)
    d_c = torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda()
    outs = [(torch.full((len(prs) * pc.RESULT_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda"),
             torch.full((len(corr),), 0x5A, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def ransac(d_r, d_i):
        fe.check(fe.lib().sd_pnp_ransac_device(len(prs), p(off), dp(d_c), p(probs), D["probability"], D["min_inliers"], D["max_iterations"], D["min_set"],
                                               D["epsilon"], D["th2"], dp(d_r), dp(d_i), None, None, 0, C.c_void_p(a.cuda_stream)))

    dev, (fr, kf) = chain["dev"], chain["slots"]
    torch.cuda.synchronize()
    ransac(*outs[0])
    ws.b.relocalize_pnp(fr, kf, chain["probs"], dev["bow"].data_ptr(), dev["kfp"].data_ptr(), dev["pts"].data_ptr(), dev["desc"].data_ptr(), rc.CAM,
                        stream=b.cuda_stream, n_points=len(chain["pts"]), **D)
    ransac(*outs[1])
    a.synchronize(); b.synchronize()
    for d_r, d_i in outs:
        assert d_r.cpu().numpy().tobytes() == want_res.tobytes() and d_i.cpu().numpy().tobytes() == want_inl.tobytes()
    for q, g in enumerate(got):
        again = ws.b.download_reloc_pnp(q)
        for k in g:
            assert np.asarray(again[k]).tobytes() == np.asarray(g[k]).tobytes(), (chain["names"][q], k)
