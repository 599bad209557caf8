"""Timing of Optimizer::PoseOptimization on the device (k_pose.h), printed as ONE JSON line:
  launch_ms        -- one sd_pose_optimize_device launch of 256 problems x 1,000 edges (60 % stereo, 30 % gross outliers, 2 deg / 5 cm
                      prior error), device events around `--launches` launches after warm-up, per launch;
  oracle_ms        -- the CPU oracle (tests/cpp/pose_oracle.cpp) on the same 256 problems over 16 host threads, wall clock;
  track_on_ms / track_off_ms / added_ms_per_step
                   -- sd_tracker_track of 256 stereo lanes (KITTI 1241x376) with the TrackWithMotionModel tail on vs off, two trackers
                      stepped alternately in one process, host clock around each (the call ends in its one synchronisation).
--launch-only runs just the launches (for `rocprofv3 --kernel-trace --stats -- python tools/bench_pose.py --launch-only`)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import pose_cases as pc  # noqa: E402


def problems(n_problems, n_edges, seed=7):
    rng = np.random.default_rng(seed)
    es, Ts = [], []
    for _ in range(n_problems):
        e, T, _ = pc.make_problem(rng, n_edges, "mixed", 0.3, noise=1.0)
        es.append(e); Ts.append(pc.perturb(T, rng, 2.0, 0.05).astype(np.float32))
    off = np.zeros(n_problems + 1, np.int32); off[1:] = np.cumsum([len(e) for e in es])
    return off, np.concatenate(es), np.stack(Ts), es


def time_launches(fe, off, edges, T0, launches, warmup):
    import torch
    L = fe.lib()
    n = len(off) - 1
    d_off = torch.from_numpy(off).cuda(); d_e = torch.from_numpy(edges.view(np.uint8)).cuda()
    d_T = torch.from_numpy(T0.reshape(n, 16)).cuda(); T_in = d_T.clone()
    d_o = torch.zeros(len(edges), dtype=torch.uint8, device="cuda"); d_g = torch.zeros(n, dtype=torch.int32, device="cuda")
    cams = np.tile(fe.camera_array(dict(pc.CAM, mb=pc.CAM["mbf"] / pc.CAM["fx"], mnMinX=0, mnMaxX=1241, mnMinY=0, mnMaxY=376)), (n, 1))
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        d_T.copy_(T_in)                                   # every launch starts from the prior
        fe.check(L.sd_pose_optimize_device(n, C.c_void_p(d_off.data_ptr()), C.c_void_p(d_e.data_ptr()), cams.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(d_T.data_ptr()), C.c_void_p(d_o.data_ptr()), C.c_void_p(d_g.data_ptr()), C.c_void_p(stream)))
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_a, copy_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_a.record()
    for _ in range(launches):
        d_T.copy_(T_in)
    copy_b.record()
    a.record()
    for _ in range(launches):
        launch()
    b.record()
    torch.cuda.synchronize()
    return (a.elapsed_time(b) - copy_a.elapsed_time(copy_b)) / launches


def time_oracle(es, T0, threads=16):
    pc.oracle()
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda k: pc.optimize(es[k], pc.CAM, T0[k]), range(len(es))))
    return (time.perf_counter() - t) * 1e3


def time_tracker(fe, synth, lanes, steps, warmup):
    import torch
    cfg = synth.KITTI_STEREO
    W, H = cfg["width"], cfg["height"]
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    pairs = {(q, t): np.stack(synth.stereo_frame(seq=q, t=t)[:2]) for q in range(8) for t in range(4)}
    frames = [torch.from_numpy(np.stack([pairs[(l % 8, t)] for l in range(lanes)])).cuda() for t in range(4)]
    trk = {on: fe.Tracker(ex, cfg, fe.SENSOR_STEREO, lanes, channels=1) for on in (True, False)}
    trk[True].set_pose_optimization(True)
    ms = {True: [], False: []}
    try:
        for k in range(warmup + steps):
            for on in ((True, False) if k % 2 == 0 else (False, True)):
                dev = frames[k % len(frames)]
                t = time.perf_counter()
                trk[on].track(dev.data_ptr(), W, W * H, [0.1 * k] * lanes)
                if k >= warmup:
                    ms[on].append((time.perf_counter() - t) * 1e3)
        ran = sum(p.ran for p in trk[True].pose_results())
    finally:
        for x in trk.values():
            x.close()
    return float(np.median(ms[True])), float(np.median(ms[False])), ran


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--edges", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launch-only", action="store_true")
    a = ap.parse_args()
    pkg = g.load_package()
    fe = pkg.frontend
    if fe.device_count() < 1:
        raise SystemExit("bench_pose needs a HIP device")
    off, edges, T0, es = problems(a.problems, a.edges)
    rec = dict(tool="bench_pose", problems=a.problems, edges_per_problem=a.edges, stereo_share=0.6, outlier_share=0.3)
    rec["launch_ms"] = round(time_launches(fe, off, edges, T0, a.launches, a.warmup), 4)
    if not a.launch_only:
        rec["oracle_ms"] = round(time_oracle(es, T0), 2)
        rec["oracle_threads"] = 16
        on, off_, ran = time_tracker(fe, pkg.synth, a.lanes, a.steps, a.warmup)
        rec.update(track_lanes=a.lanes, track_on_ms=round(on, 3), track_off_ms=round(off_, 3), added_ms_per_step=round(on - off_, 3),
                   lanes_that_ran_pose=int(ran))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
