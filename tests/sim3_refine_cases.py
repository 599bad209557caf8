"""Shared by test_gpu_sim3_refine.py, tools/fuzz_sim3_opt.py and tools/bench_sim3_opt.py: scenes for sd_batch_compute_sim3_refine, built
as tests/sim3_cases.py builds its SearchBySim3 scenes (two keyframes per job seeing one cloud, a map point in either map, features with
pixel noise), plus what the chain reads beside them -- the KF-KF BoW matches (the scene's `matched12`), a RANSAC answer per job and the
RANSAC's correspondence tags and inlier bytes -- and a plain numpy restatement of every stage but the search and the optimiser, which
have their own oracles (sim3_cases.cpu_search, sim3_opt_cases.solve)."""
import numpy as np

import sim3_cases as s3
import sim3_opt_cases as so

F32 = np.float32


def refine_scene(seed, n_points=300, n_jobs=3, not_found=(), prior_noise=0.01, inlier_share=0.85, noise=0.7):
    """random_search_scene(seed) with, per job, `ransac` (sim3_cases.RESULT_DTYPE: found, and R12 / t12 / s12 = the scene's similarity
    rotated by prior_noise rad), `tags` (the i1 carrying a BoW match, in order) and `inl` (u8 per tag).  Jobs in not_found get found = 0."""
    sc = s3.random_search_scene(seed, n_points, n_jobs, noise=noise)
    rng = np.random.default_rng([808, seed, n_points, n_jobs])
    for q, pr in enumerate(sc["pairs"]):
        r = np.zeros((), s3.RESULT_DTYPE)
        r["found"] = int(q not in not_found); r["no_more"] = 1 - r["found"]; r["iteration"] = 3; r["n_inliers"] = 25; r["max_its"] = 300
        R = so.rot(rng.normal(size=3), prior_noise) @ np.asarray(pr["R12"], np.float64).reshape(3, 3)
        r["R12"] = R.astype(F32).reshape(-1); r["t12"] = np.asarray(pr["t12"], F32).reshape(3); r["s12"] = F32(pr["s12"])
        T = np.eye(4, dtype=F32); T[:3, :3] = F32(r["s12"]) * R.astype(F32); T[:3, 3] = r["t12"]
        r["T12"] = T.reshape(-1)
        pr["ransac"] = r
        pr["tags"] = np.nonzero(np.asarray(pr["matched12"]) != -1)[0].astype(np.int32)
        pr["inl"] = (rng.random(len(pr["tags"])) < inlier_share).astype(np.uint8)
    sc["name"] = "refine_%d_%d" % (seed, n_points)
    return sc


def device_refine(ws, scene, fix_scale=False, th2=10.0, cam=s3.CAM, upload=True, timed=None):
    """One sd_batch_compute_sim3_refine for all jobs of the scene -> per job dict(result, final12, merged12, corr, state, add12, n_found)."""
    import torch
    if upload:
        ws.upload_grid(scene["kfs"], cam)
    prs = scene["pairs"]
    n = len(prs)
    t1 = np.full((n, ws.cap), -1, np.int32); t2 = np.full((n, ws.cap), -1, np.int32); tm = np.full((n, ws.cap), -1, np.int32)
    for q, pr in enumerate(prs):
        t1[q, :len(pr["p1"])] = pr["p1"]; t2[q, :len(pr["p2"])] = pr["p2"]; tm[q, :len(pr["matched12"])] = pr["matched12"]
    off = np.concatenate([[0], np.cumsum([len(pr["tags"]) for pr in prs])]).astype(np.int32)
    rc = np.zeros(max(int(off[-1]), 1), s3.CORR_DTYPE)
    rc["tag"][:off[-1]] = np.concatenate([pr["tags"] for pr in prs])
    inl = np.zeros(max(int(off[-1]), 1), np.uint8); inl[:off[-1]] = np.concatenate([pr["inl"] for pr in prs])
    ran = np.array([pr["ransac"] for pr in prs], s3.RESULT_DTYPE)
    dev = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()     # noqa: E731
    d1, d2, dm, d_rc, d_inl, d_ran = dev(t1), dev(t2), dev(tm), dev(rc), dev(inl), dev(ran)
    pts = np.ascontiguousarray(scene["points"], s3.MP_DTYPE)
    d_pts, d_desc = dev(pts), dev(np.ascontiguousarray(scene["pdesc"], np.uint8))
    kf = scene["kfs"]
    def call():
        ws.b.compute_sim3_refine([pr["k1"] for pr in prs], [pr["k2"] for pr in prs], np.array([kf[pr["k1"]]["Tcw"] for pr in prs], F32).reshape(n, 16),
                                 np.array([kf[pr["k2"]]["Tcw"] for pr in prs], F32).reshape(n, 16), d_ran.data_ptr(), off, d_rc.data_ptr(), d_inl.data_ptr(),
                                 dm.data_ptr(), cam, d_pts.data_ptr(), d_desc.data_ptr(), d1.data_ptr(), d2.data_ptr(), th=scene.get("th", s3.TH_SIM3),
                                 th2=th2, fix_scale=fix_scale, n_points=len(pts))
    call()
    if timed is not None:                                        # a benchmark: the caller times further calls, the tables stay alive in it
        timed.append(call); timed.append((d1, d2, dm, d_rc, d_inl, d_ran, d_pts, d_desc))
    out = []
    for q, pr in enumerate(prs):
        res, f12 = ws.b.download_sim3_refine(q)
        m, corr, st = ws.b.download_sim3_refine_stages(q)
        a12, _, _, nf = ws.b.download_sim3_matches(q)
        out.append(dict(result=res, final12=f12, merged12=m, corr=corr, state=st, add12=a12, n_found=nf))
    return out


def cpu_refine(scene, lv, cap, fix_scale=False):
    """The whole chain on the CPU (numpy stages, the two oracles), free-running: per job dict(ret, added, added_then_removed, minus2)."""
    out = []
    for pr in scene["pairs"]:
        N1 = len(pr["p1"])
        if not pr["ransac"]["found"]:
            out.append(dict(ret=0, added=0, added_then_removed=0, minus2=0, ran=0))
            continue
        merged = np_merged(pr, cap)
        one = dict(scene, pairs=[dict(pr, matched12=merged[:N1].copy(), s12=pr["ransac"]["s12"], R12=pr["ransac"]["R12"], t12=pr["ransac"]["t12"])])
        add = np.full(cap, -1, np.int32); add[:N1] = s3.cpu_search(one, lv=lv)[0][0][0]
        corr, after = np_build(scene, pr, merged, add, lv)
        r, st = so.solve(opt_case(scene, pr, corr, fix_scale=fix_scale))[:2]
        removed = np.zeros(N1, bool); removed[corr["tag"][st != 0]] = True
        out.append(dict(ret=int(r["ret"]), added=int((add >= 0).sum()), added_then_removed=int(((add[:N1] >= 0) & removed).sum()),
                        minus2=int((after == -2).sum()), ran=1))
    return out


def np_merged(pr, cap):
    """Step 1: vpMapPointMatches[i1] = vbInliers ? the BoW match : NULL, as a matched12 row of `cap` entries."""
    m = np.full(cap, -1, np.int32)
    if pr["ransac"]["found"]:
        t = pr["tags"][pr["inl"] != 0]
        m[t] = np.asarray(pr["matched12"], np.int32)[t]
    return m


def np_build(scene, pr, merged12, add12, lv):
    """Step 3 from the device's own merged12 and add12 rows: (correspondences (SIM3_OPT_CORR), vpMapPointMatches after the merge)."""
    a, b = scene["kfs"][pr["k1"]], scene["kfs"][pr["k2"]]
    N1, N2 = len(a["kp"]), len(b["kp"])
    inv = (F32(1.0) / np.asarray(lv.sigma2, F32)).astype(F32)
    after = np.where(add12[:N1] >= 0, add12[:N1], merged12[:N1]).astype(np.int32)
    if not pr["ransac"]["found"]:
        return np.zeros(0, so.CORR_DTYPE), after
    p1 = np.asarray(pr["p1"], np.int64)[:N1]; p2t = np.asarray(pr["p2"], np.int64)
    ok2 = (after >= 0) & (after < N2)
    p2 = np.where(ok2, p2t[np.where(ok2, after, 0)], -1) if N2 else np.full(N1, -1)
    i1 = np.nonzero(ok2 & (p1 >= 0) & (p2 >= 0))[0]                      # the `continue`s of Optimizer.cc:1101-1136, in i1 order
    i2 = after[i1]
    c = np.zeros(len(i1), so.CORR_DTYPE)
    c["xw1"] = scene["points"]["xw"][p1[i1]]; c["xw2"] = scene["points"]["xw"][p2[i1]]
    c["obs1"] = np.stack([a["kp"]["x"][i1], a["kp"]["y"][i1]], 1); c["obs2"] = np.stack([b["kp"]["x"][i2], b["kp"]["y"][i2]], 1)
    c["inv_sigma2_1"] = inv[a["kp"]["octave"][i1]]; c["inv_sigma2_2"] = inv[b["kp"]["octave"][i2]]; c["tag"] = i1
    return c, after


def opt_case(scene, pr, corr, cam=s3.CAM, fix_scale=False, th2=10.0):
    """The optimiser's problem of a job over the given correspondences, as a sim3_opt_cases case."""
    p = np.zeros((), so.PROBLEM_DTYPE)
    p["Tcw1"] = np.asarray(scene["kfs"][pr["k1"]]["Tcw"], F32).reshape(-1); p["Tcw2"] = np.asarray(scene["kfs"][pr["k2"]]["Tcw"], F32).reshape(-1)
    K = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], F32)
    p["K1"] = K; p["K2"] = K; p["R12"] = pr["ransac"]["R12"]; p["t12"] = pr["ransac"]["t12"]; p["s12"] = pr["ransac"]["s12"]
    p["th2"] = th2; p["fix_scale"] = int(fix_scale)
    return dict(name="job", corr=corr, prob=p, expect={}, exact=True)


def np_scw(opt, Tcw2):
    """Step 6 in numpy f64: (s R | t) of gScm * gSmw with gSmw = (R2w, t2w, 1)."""
    T2 = np.asarray(Tcw2, np.float64).reshape(4, 4)
    R, t, s = so.quat_to_R(np.asarray(opt["q"])), np.asarray(opt["t"]), float(opt["s"])
    return R @ T2[:3, :3], s * (R @ T2[:3, 3]) + t, s


def check_refine(ws, scene, fix_scale=False):
    """Runs the chain on the device and holds every stage to its reference, each from the device's own stage input (see
    tests/test_gpu_sim3_refine.py); -> (per-job downloads, what the scene reached)."""
    got = device_refine(ws, scene, fix_scale=fix_scale)
    seen = dict(ret=[], minus2=0, added_then_removed=0, added=0, not_run=0)
    for q, (pr, g) in enumerate(zip(scene["pairs"], got)):
        name = "%s job %d" % (scene["name"], q)
        res, N1 = g["result"], len(pr["p1"])
        found = bool(pr["ransac"]["found"])
        assert bool(res["ran"]) == found, name
        # 1. the inlier merge
        assert np.array_equal(g["merged12"], np_merged(pr, ws.cap)), name
        if not found:                                           # nothing runs: no search, no correspondence, ret 0, every match NULL
            assert g["n_found"] == 0 and (g["add12"] == -1).all() and len(g["corr"]) == 0 and res["opt"]["ret"] == 0 and res["matched"] == 0, name
            assert (g["final12"] == -1).all(), name
            seen["not_run"] += 1
            continue
        # 2. SearchBySim3 from the device's own merged row and the RANSAC's similarity: byte for byte
        one = dict(scene, pairs=[dict(pr, matched12=g["merged12"][:N1].copy(), s12=pr["ransac"]["s12"], R12=pr["ransac"]["R12"], t12=pr["ransac"]["t12"])])
        want = s3.cpu_search(one, lv=ws.lv)[0][0]
        assert g["add12"][:N1].tobytes() == want[0].tobytes() and g["n_found"] == want[3] and (g["add12"][N1:] == -1).all(), name
        # 3. the correspondences from the device's own rows: byte for byte
        corr, after = np_build(scene, pr, g["merged12"], g["add12"], ws.lv)
        assert res["n_built"] == len(corr) == len(g["corr"]) and g["corr"].tobytes() == corr.tobytes(), name
        # 4. the optimiser on the device's own correspondences
        case = opt_case(scene, pr, g["corr"], fix_scale=fix_scale)
        w_res, w_st = so.solve(case, so.WAVE)[:2]
        assert res["opt"].tobytes() == w_res.tobytes() and g["state"].tobytes() == w_st.tobytes(), (name, res["opt"], w_res)
        s_res, s_st = so.solve(case)[:2]
        assert (s_res["ret"], s_res["n_bad"], s_res["more_iterations"], s_res["written"]) == \
               (res["opt"]["ret"], res["opt"]["n_bad"], res["opt"]["more_iterations"], res["opt"]["written"]) and np.array_equal(s_st, g["state"]), name
        # 5. the final matches and the gate
        final = np.full(ws.cap, -1, np.int32); final[:N1] = after
        final[g["corr"]["tag"][g["state"] != 0]] = -1
        assert np.array_equal(g["final12"], final), name
        assert res["matched"] == int(res["opt"]["ret"] >= 20), name
        # 6. Scw = gScm * gSmw
        R, t, s = np_scw(res["opt"], scene["kfs"][pr["k2"]]["Tcw"])
        assert np.allclose(so.quat_to_R(res["Scw_q"]), R, atol=1e-12) and np.allclose(res["Scw_t"], t, rtol=1e-12, atol=1e-12), name
        assert abs(res["Scw_s"] - s) <= 1e-15 * abs(s), name
        M = np.eye(4); M[:3, :3] = s * R; M[:3, 3] = t
        assert np.allclose(res["Scw"].reshape(4, 4), M, rtol=3e-7, atol=1e-6), name
        added = g["add12"][:N1] >= 0
        seen["ret"].append(int(res["opt"]["ret"])); seen["added"] += int(added.sum())
        seen["minus2"] += int((after == -2).sum())
        removed = np.zeros(N1, bool); removed[g["corr"]["tag"][g["state"] != 0]] = True
        seen["added_then_removed"] += int((added & removed).sum())
        assert ((final[:N1] == -2) == (after == -2)).all(), name        # a match that is not in KF2 has no edge and stays
    return got, seen
