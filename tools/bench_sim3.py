"""Timing of LoopClosing::ComputeSim3's two data-parallel stages on the device (k_sim3.h), written to profiles/sim3_bench.json and
printed as ONE JSON line.
  ransac -- `--keyframes` x `--candidates` Sim3Solver problems of `--correspondences` correspondences (a third of them with 30 %, a
            third with 60 % outliers), SetRansacParameters(0.99, 20, `--iterations`): ONE sd_sim3_ransac_device call, HIP events around
            `--calls` calls after warm-up (the free function keeps no per-kernel clock: per call only); the sequential CPU oracle
            (tests/cpp/sim3_oracle.cpp) on the same problems, one C loop over a contiguous chunk of problems per host thread, on 1 and
            on 16 threads, wall clock, median of five; results compared byte for byte.
  search -- `--pairs` SearchBySim3 pairs at about `--features` features a keyframe (8 distinct keyframe pairs, repeated), th = 7.5: ONE
            sd_batch_search_by_sim3 call, a host clock around calls that end in the workspace's stream synchronise, the three kernels'
            times from sd_batch_kernel_times in a pass of their own; the oracle as above.
No threshold is set on either ratio."""
import argparse
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
import triangulate_cases as tc  # noqa: E402
import fuse_cases as fc  # noqa: E402
import sim3_cases as sc  # noqa: E402

GEOM = dict(W=1241, H=376, nfeatures=2000, scale=1.2, nlevels=8)


def bench_ransac(fe, a):
    import torch
    n = a.keyframes * a.candidates
    probs = [sc.make_problem(9000 + k, a.correspondences, s=1.0 + 0.01 * (k % 7), outliers=(0.0, 0.3, 0.6)[k % 3], noise=0.002,
                             max_iterations=a.iterations) for k in range(n)]
    off, corr, tab = sc.pack(probs)
    d_c = torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda()
    d_r = torch.zeros(n * sc.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda"); d_i = torch.zeros(len(corr), dtype=torch.uint8, device="cuda")
    L = fe.lib()
    stream = torch.cuda.current_stream().cuda_stream
    C = fe.C

    def call():
        fe.check(L.sd_sim3_ransac_device(n, fe._p(off), C.c_void_p(d_c.data_ptr()), fe._p(tab), 0.99, 20, a.iterations, C.c_void_p(d_r.data_ptr()),
                                         C.c_void_p(d_i.data_ptr()), None, C.c_void_p(stream)))
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        call()
    e1.record(); torch.cuda.synchronize()
    call_ms = e0.elapsed_time(e1) / a.calls
    res = d_r.cpu().numpy().view(sc.RESULT_DTYPE); inl = d_i.cpu().numpy()
    # the oracle: tables marshalled once, one C loop over a contiguous chunk of problems per host thread (a call per problem from a
    # Python thread pool spends its time under the interpreter lock and measures one thread); the median of five runs each
    sc.find_packed(off, corr, tab, 0.99, 20, a.iterations, 16)
    times = {}
    for threads in (1, 16):
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            o_res, o_inl, o_info = sc.find_packed(off, corr, tab, 0.99, 20, a.iterations, threads)
            ts.append((time.perf_counter() - t) * 1e3)
        times[threads] = sorted(ts)[2]
    oracle_ms = times[16]
    same = all(sc.same_result(res[k], o_res[k]) for k in range(n)) and inl.tobytes() == o_inl.tobytes()
    hyp_dev = int(res["max_its"].sum()); hyp_seq = int(o_info[:, 1].sum())
    return dict(problems=n, correspondences=a.correspondences, max_iterations=a.iterations, found=int(res["found"].sum()),
                hypotheses_device=hyp_dev, hypotheses_sequential=hyp_seq, call_ms=round(call_ms, 4), oracle_ms=round(oracle_ms, 3),
                oracle_threads=16, oracle_ms_one_thread=round(times[1], 3), host_cpus=len(os.sched_getaffinity(0)), identical_to_oracle=bool(same))


def bench_search(fe, synth, a):
    import torch
    distinct = 8
    scene = sc.random_search_scene(77, a.features, distinct)           # at most one feature per point and keyframe
    ws = fc.Workspace(fe, 2 * distinct, tc.vocabulary(synth, 5), GEOM)
    assert max(len(k["kp"]) for k in scene["kfs"]) <= ws.cap
    scene["pairs"] = [scene["pairs"][q % distinct] for q in range(a.pairs)]
    got = sc.device_search(ws, scene)                                        # uploads, runs once, downloads
    prs = scene["pairs"]
    n = len(prs)
    t1 = np.full((n, ws.cap), -1, np.int32); t2 = np.full((n, ws.cap), -1, np.int32); tm = np.full((n, ws.cap), -1, np.int32)
    for q, pr in enumerate(prs):
        t1[q, :len(pr["p1"])] = pr["p1"]; t2[q, :len(pr["p2"])] = pr["p2"]; tm[q, :len(pr["matched12"])] = pr["matched12"]
    d1, d2, dm = torch.from_numpy(t1).cuda(), torch.from_numpy(t2).cuda(), torch.from_numpy(tm).cuda()
    d_pts = torch.from_numpy(np.frombuffer(scene["points"].tobytes(), np.uint8).copy()).cuda()
    d_desc = torch.from_numpy(scene["pdesc"].reshape(-1).copy()).cuda()
    kf = scene["kfs"]
    args = ([pr["k1"] for pr in prs], [pr["k2"] for pr in prs], np.array([kf[pr["k1"]]["Tcw"] for pr in prs], np.float32).reshape(n, 16),
            np.array([kf[pr["k2"]]["Tcw"] for pr in prs], np.float32).reshape(n, 16), [pr["s12"] for pr in prs],
            np.array([pr["R12"] for pr in prs], np.float32).reshape(n, 9), np.array([pr["t12"] for pr in prs], np.float32).reshape(n, 3), tc.CAM,
            d_pts.data_ptr(), d_desc.data_ptr(), d1.data_ptr(), d2.data_ptr(), dm.data_ptr())

    def call():
        ws.b.search_by_sim3(*args, th=sc.TH_SIM3, n_points=len(scene["points"]))
    for _ in range(a.warmup):
        call()
    ws.b.sync()
    t = time.perf_counter()
    for _ in range(a.calls):
        call()
    ws.b.sync()
    call_ms = (time.perf_counter() - t) * 1e3 / a.calls
    ws.b.set_profiling(True); ws.b.reset_kernel_times()
    for _ in range(a.calls):
        call()
    ws.b.sync()
    kt = ws.b.kernel_times()
    ws.b.set_profiling(False)
    singles = [dict(scene, pairs=[pr]) for pr in prs]
    sc.cpu_search(singles[0], lv=ws.lv)
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        ref = list(pool.map(lambda s: sc.cpu_search(s, lv=ws.lv)[0][0], singles))
    oracle_ms = (time.perf_counter() - t) * 1e3
    same = all(all(x[k].tobytes() == y[k].tobytes() for k in range(3)) and x[3] == y[3] for x, y in zip(got, ref))
    rec = dict(pairs=n, distinct_pairs=distinct, features=int(np.mean([len(k["kp"]) for k in kf])), found=int(sum(x[3] for x in got)),
               call_ms=round(call_ms, 4), kernel_ms={k: round(kt[k][0] / max(kt[k][1], 1), 4) for k in ("k_sim3_mark", "k_sim3_search", "k_sim3_agree")},
               oracle_ms=round(oracle_ms, 2), oracle_threads=16, identical_to_oracle=bool(same))
    ws.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--correspondences", type=int, default=150)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("ransac", "search"), default=None, help="one stage only (a profiler run); nothing is written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_bench.json"))
    a = ap.parse_args()
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    if fe.device_count() < 1:
        raise SystemExit("bench_sim3 needs a HIP device")
    if a.only:
        print(json.dumps({a.only: bench_ransac(fe, a) if a.only == "ransac" else bench_search(fe, synth, a)}))
        return
    rec = dict(tool="bench_sim3", timed_calls=a.calls, ransac=bench_ransac(fe, a), search=bench_search(fe, synth, a))
    for k in ("ransac", "search"):
        rec[k]["oracle_over_device"] = round(rec[k]["oracle_ms"] / rec[k]["call_ms"], 2)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
