"""Optimizer::PoseOptimization on the GPU (k_pose.h through sd_pose_optimize_*, sd_batch_pose_optimize and the tracker's
TrackWithMotionModel tail) against the CPU oracle tests/cpp/pose_oracle.cpp."""
import numpy as np
import pytest

import pose_cases as pc

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 5, 9, 10, 11, 37, 64, 257, 1000, 2000, 8000)


def _suite():
    rng = np.random.default_rng(2024)
    probs = []
    for n in SIZES:
        for kind in ("mono", "stereo", "mixed"):
            for ratio in (0.0, 0.3, 0.6):
                for pert in ((0, 0), (2, 0.05), (10, 0.5)):
                    e, T, _ = pc.make_problem(rng, n, kind, ratio, noise=1.0)
                    probs.append((e, pc.perturb(T, rng, *pert).astype(np.float32)))
    return probs


def _pack(probs):
    off = np.zeros(len(probs) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e, _ in probs])
    edges = np.concatenate([e for e, _ in probs]) if off[-1] else np.zeros(0, pc.EDGE_DTYPE)
    return off, edges, np.stack([T for _, T in probs])


def test_plain_abi_matches_oracle(gpu, fe):
    probs = _suite()
    off, edges, T0 = _pack(probs)
    T, out, good = fe.pose_optimize(off, edges, pc.CAM, T0)
    T2, out2, good2 = fe.pose_optimize(off, edges, pc.CAM, T0)
    assert T.tobytes() == T2.tobytes() and out.tobytes() == out2.tobytes() and good.tobytes() == good2.tobytes(), "two runs differ"
    bad = []
    for k, (e, Tk) in enumerate(probs):
        r, To, oo, _ = pc.optimize(e, pc.CAM, Tk)
        og = out[off[k]:off[k + 1]]
        if r != good[k] or not np.array_equal(oo, og) or not pc.pose_close(T[k], To):
            bad.append((k, len(e), r, int(good[k]), int(np.sum(oo != og)), float(np.abs(T[k] - To).max())))
    assert not bad, "%d of %d problems differ from the oracle, first: %r" % (len(bad), len(probs), bad[:5])
    for k in range(0, len(probs), 37):                       # alone == batched, bit for bit
        e, Tk = probs[k]
        Ta, oa, ga = fe.pose_optimize(np.array([0, len(e)], np.int32), e, pc.CAM, Tk[None])
        assert Ta[0].tobytes() == T[k].tobytes() and oa.tobytes() == out[off[k]:off[k + 1]].tobytes() and ga[0] == good[k], k


def test_ground_truth_with_gross_outliers(gpu, fe):
    rng = np.random.default_rng(77)
    probs, truth, gross = [], [], []
    for kind in ("mono", "stereo", "mixed"):
        for n in (100, 1000):
            e, T, bad = pc.make_problem(rng, n, kind, 0.3, noise=0.0, gross=20.0)
            probs.append((e, pc.perturb(T, rng, 2.0, 0.05).astype(np.float32))); truth.append(T); gross.append(bad)
    off, edges, T0 = _pack(probs)
    T, out, good = fe.pose_optimize(off, edges, pc.CAM, T0)
    for k in range(len(probs)):
        assert pc.pose_close(T[k], truth[k], 1e-5), (k, np.abs(T[k] - truth[k]).max())
        o = out[off[k]:off[k + 1]].astype(bool)
        assert o[gross[k]].all(), k
        assert good[k] == len(o) - o.sum()


def test_workspace_path_matches_oracle(gpu, fe, synth):
    """extract -> stereo -> unproject -> grid -> SearchByProjection -> PoseOptimization on the device, against the oracle fed with the
    downloaded mvKeysUn / mvuRight / octave / xw[match] (the construction of test_gpu_match.py's `seq` fixture)."""
    cfg = synth.KITTI_STEREO
    T = 3
    frames = [synth.stereo_frame(seq=5, t=t) for t in range(T)]
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], 2 * T)
    try:
        b.extract_host(np.stack([im for (l, r, _) in frames for im in (l, r)]))
        b.stereo_match(T, cfg["bf"], cfg["fx"])
        cam = fe.make_camera(cfg)
        b.assign_grid(2 * T, cam)
        I = np.eye(4, dtype=np.float32)
        b.unproject(2, T, cam, np.tile(I, (T, 1, 1)))
        b.search_by_projection([2, 4], [0, 2], np.stack([I, I]), np.stack([I, I]), cam, 15.0)
        prior = np.stack([I, I]); prior[1, 0, 3] = 0.01
        b.pose_optimize([0, 1], Tcw=prior)
        inv = ex.mvInvLevelSigma2
        for p, (cur, last) in enumerate(((1, 0), (2, 1))):
            m, _, nm = b.download_matches(p)
            assert nm > 100
            Tg, og, ni, ng = b.download_pose(p)
            kp = b.download_keys_un(2 * cur)
            ur, _, _ = b.download_stereo(cur)
            xw, _ = b.download_mappoints(2 * last)
            idx = np.nonzero(m[:len(kp)] >= 0)[0]
            e = np.zeros(len(idx), pc.EDGE_DTYPE)
            e["xw"] = xw[m[idx]]; e["u"] = kp["x"][idx]; e["v"] = kp["y"][idx]; e["ur"] = ur[idx]
            e["inv_sigma2"] = inv[kp["octave"][idx]]; e["kp_index"] = idx
            r, To, oo, _ = pc.optimize(e, dict(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], mbf=cam["mbf"]), prior[p])
            assert ni == len(idx) and ng == r
            assert np.array_equal(og[idx], oo) and not og[np.setdiff1d(np.arange(len(og)), idx)].any()
            assert pc.pose_close(Tg, To)
    finally:
        b.close()


def _lane_images(synth, cfg, sensor, l, t):
    """Lane 0: a plain sequence.  Lane 1: every frame 30 px further right.  Lane 2: 20 px per frame, and frame 3 a featureless (uniform)
    image: no matches, so the 2*th retry runs and the device gate keeps the pose solver off the lane."""
    seq, shift = 3 + l, (0, 30, 20)[l] * t
    if sensor == "stereo":
        a, b, _ = synth.stereo_frame(seq=seq, t=t)
        ims = [np.roll(a, shift, 1), np.roll(b, shift, 1)]
    else:
        c, d, _ = synth.rgbd_frame(seq, t, cfg)
        ims = [np.roll(c, shift, 1), np.roll(d, shift, 1)]
    if l == 2 and t == 3:
        ims[0] = np.full_like(ims[0], 128)
        if sensor == "stereo":
            ims[1] = np.full_like(ims[1], 128)
    return ims


def _run_tracker(fe, synth, sensor, pose_on, with_map=False, frames=5, lanes=3):
    """with_map: after every step the lane's mLastFrame points get flag bit1 (Observations() > 0) through sd_tracker_set_mappoints."""
    import torch
    s = fe.SENSOR_STEREO if sensor == "stereo" else fe.SENSOR_RGBD
    cfg = synth.KITTI_STEREO if sensor == "stereo" else synth.KITTI03_RGBD
    W, H = cfg["width"], cfg["height"]
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    trk = fe.Tracker(ex, cfg, s, lanes, channels=1 if sensor == "stereo" else 3)
    if pose_on:
        trk.set_pose_optimization(True)
    out = []
    try:
        prev_last = [None] * lanes
        for t in range(frames):
            ims = [_lane_images(synth, cfg, sensor, l, t) for l in range(lanes)]
            if sensor == "stereo":
                dev = torch.from_numpy(np.stack([np.stack(p) for p in ims])).cuda()
                R = trk.track(dev.data_ptr(), W, W * H, [0.1 * t] * lanes)
            else:
                rgb = torch.from_numpy(np.ascontiguousarray(np.stack([p[0] for p in ims]))).cuda()
                dep = torch.from_numpy(np.ascontiguousarray(np.stack([p[1] for p in ims])).view(np.int16)).cuda()
                R = trk.track(rgb.data_ptr(), W * 3, W * H * 3, [0.1 * t] * lanes, d_depth=dep.data_ptr(), depth_stride=W, depth_pitch=W * H)
            step = dict(res=[], pose=None, frames=[], data=[])
            for l in range(lanes):
                r = R[l]
                step["res"].append({f: (np.array(getattr(r, f)).tobytes() if not isinstance(getattr(r, f), int) else getattr(r, f))
                                    for f, _ in fe.LaneResult._fields_})
                kp, desc, _ = trk.batch.download(r.cur_slot)
                step["frames"].append(kp.tobytes() + desc.tobytes())
                if pose_on and prev_last[l] is not None:
                    m, _, nm = trk.batch.download_matches(lanes + l)
                    kpu = trk.batch.download_keys_un(r.cur_slot)
                    ur, _ = trk.batch.download_rgbd(r.cur_slot)
                    xw, fl = trk.batch.download_mappoints(prev_last[l])
                    _, og, _, _ = trk.batch.download_pose(lanes + l)
                    step["data"].append((m, nm, kpu, ur, xw, fl, og))
                else:
                    step["data"].append(None)
                prev_last[l] = r.last_slot
            if pose_on:
                step["pose"] = [(np.array(p.Tcw, np.float32).reshape(4, 4), p.ran, p.n_matches, p.n_initial, p.n_good, p.n_matches_map, p.ok)
                                for p in trk.pose_results()]
            if with_map:
                xs, fs = [], []
                for l in range(lanes):
                    xw, fl = trk.batch.download_mappoints(R[l].last_slot)
                    n = R[l].N
                    fl = fl[:n].copy(); fl[(fl & 1) != 0] |= 2
                    xs.append(xw[:n]); fs.append(fl)
                trk.set_mappoints(xs, fs)
            out.append(step)
    finally:
        trk.close()
    return out, ex, cfg


def _check_against_oracle(run, ex, cfg, fe, off=None):
    """Every sd_pose_result of a pose-mode run against the oracle on the downloaded matches; returns counters of what was exercised."""
    cam = fe.make_camera(cfg)
    c5 = dict(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], mbf=cam["mbf"])
    seen = dict(ran=0, gated=0, recovered=0, map_ok=0)
    for t, a in enumerate(run):
        for l in range(len(a["res"])):
            Tp, ran, nmat, ni, ng, nmap, ok = a["pose"][l]
            d = a["data"][l]
            if d is None:
                assert ran == 0 and nmat == -1
                continue
            m, nm, kpu, ur, xw, fl, og = d
            assert nmat == nm and a["res"][l]["n_last_matches"] == nm
            assert (ran == 0) == (nm < 20), (t, l, nm, ran)
            if off is not None:
                nm_off = off[t]["res"][l]["n_last_matches"]
                if nm_off >= 20:
                    assert nm == nm_off, (t, l)                # no retry: the matches of the mode off
                elif nm >= 20:
                    seen["recovered"] += 1                    # the 2*th retry brought the lane over 20
            if not ran:
                seen["gated"] += 1                             # the device gate (k_pose_edges) kept the solver off this lane
                assert ni == 0 and ng == 0 and not og.any()
                continue
            seen["ran"] += 1
            idx = np.nonzero(m[:len(kpu)] >= 0)[0]
            e = np.zeros(len(idx), pc.EDGE_DTYPE)
            e["xw"] = xw[m[idx]]; e["u"] = kpu["x"][idx]; e["v"] = kpu["y"][idx]; e["ur"] = ur[idx]
            e["inv_sigma2"] = ex.mvInvLevelSigma2[kpu["octave"][idx]]; e["kp_index"] = idx
            r, To, oo, _ = pc.optimize(e, c5, np.eye(4, dtype=np.float32))
            assert ni == len(idx) and ng == r and pc.pose_close(Tp, To), (t, l)
            assert np.array_equal(og[idx], oo), (t, l)
            nmap_o = int(np.sum((oo == 0) & ((fl[m[idx]] & 2) != 0)))     # TrackWithMotionModel's nmatchesMap
            assert nmap == nmap_o and ok == int(nmap_o >= 10), (t, l, nmap, nmap_o, ok)
            seen["map_ok"] += ok
    return seen


@pytest.mark.parametrize("sensor", ["stereo", "rgbd"])
def test_tracker_pose_mode_matches_oracle_and_changes_nothing_else(gpu, fe, synth, sensor):
    on, ex, cfg = _run_tracker(fe, synth, sensor, True)
    off, _, _ = _run_tracker(fe, synth, sensor, False)
    for t, (a, b) in enumerate(zip(on, off)):
        assert a["frames"] == b["frames"], t
        for l in range(len(a["res"])):
            for f in a["res"][l]:
                if f != "n_last_matches":
                    assert a["res"][l][f] == b["res"][l][f], (t, l, f)
    seen = _check_against_oracle(on, ex, cfg, fe, off)
    assert seen["ran"] > 0 and seen["gated"] > 0, seen
    assert seen["map_ok"] == 0                                 # sharded batch mode: the frame's own points have no observations


def test_tracker_pose_mode_counts_points_with_observations(gpu, fe, synth):
    """With the caller's MapPoints (flag bit1 = Observations() > 0, sd_tracker_set_mappoints) nmatchesMap counts the inliers among them and
    TrackWithMotionModel returns ok = nmatchesMap >= 10."""
    run, ex, cfg = _run_tracker(fe, synth, "stereo", True, with_map=True)
    seen = _check_against_oracle(run, ex, cfg, fe)
    assert seen["map_ok"] > 0 and seen["ran"] > 0, seen


def test_cpp_optimizer_mirror_matches_oracle(gpu, fe, tmp_path):
    """host/Optimizer.h (ORB_SLAM2::Optimizer::PoseOptimization over the C ABI), built with g++ against the library: the return value,
    mTcw and mvbOutlier equal the oracle's; keypoints without a MapPoint keep their mvbOutlier."""
    import os
    import subprocess
    exe = str(tmp_path / "pose_mirror")
    libdir = os.path.join(pc.ROOT, "slam-dynamic_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(pc.ROOT, "include"),
                           "-I" + os.path.join(pc.ROOT, "slam-dynamic_amd", "host"), os.path.join(pc.ROOT, "tests/cpp/pose_mirror_main.cpp"),
                           "-L" + libdir, "-lsd_frontend", "-Wl,-rpath," + libdir, "-o", exe])
    rng = np.random.default_rng(31)
    n = 700
    e, T, _ = pc.make_problem(rng, n, "mixed", 0.3, noise=1.0)
    inv = (1.0 / (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)).astype(np.float32)
    e["inv_sigma2"] = inv[np.arange(n) % 8]                       # the mirror's frame takes octave = i % 8
    has = rng.random(n) < 0.7
    T0 = pc.perturb(T, rng, 2.0, 0.05).astype(np.float32)
    rec = np.zeros(n, [("has", "<i4"), ("xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv", "<f4")])
    rec["has"] = has; rec["xw"] = e["xw"]; rec["u"] = e["u"]; rec["v"] = e["v"]; rec["ur"] = e["ur"]; rec["inv"] = e["inv_sigma2"]
    blob = np.int32(n).tobytes() + pc.cam5(pc.CAM).tobytes() + T0.tobytes() + rec.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = (tmp_path / "out.bin").read_bytes()
    ret = int(np.frombuffer(out, np.int32, 1)[0])
    Tm = np.frombuffer(out, np.float32, 16, 4).reshape(4, 4)
    flags = np.frombuffer(out, np.uint8, n, 68)
    r, To, oo, _ = pc.optimize(e[has], pc.CAM, T0)
    assert ret == r and pc.pose_close(Tm, To) and np.array_equal(flags[has], oo)
    assert flags[~has].all()
