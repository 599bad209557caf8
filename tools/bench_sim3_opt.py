#!/usr/bin/env python3
"""Timing of Optimizer::OptimizeSim3 on the device (k_sim3_opt.h), written to profiles/sim3_opt_bench.json and printed as ONE JSON line.
`--keyframes` x `--candidates` problems of about `--correspondences` correspondences (10 % outliers, a 0.02 rad / 0.1 / 3 % prior):
ONE sd_sim3_optimize_device call, HIP events around `--calls` calls after warm-up, the median of `--runs` such measurements; the
sequential CPU oracle (tests/cpp/sim3_opt_oracle.cpp, the kernel's summation order) on the same problems, one C loop over a contiguous
chunk of problems per host thread, on 1 and on 16 threads, wall clock, median of five; results compared byte for byte.  A single
problem is timed the same way (`single`), which is where the host is closest.
`chain`: sd_batch_compute_sim3_refine on `--pairs` jobs at about `--features` features a keyframe (8 distinct keyframe pairs, repeated):
a host clock around calls that end in the workspace's stream synchronise; the CPU chain (numpy stages, the SearchBySim3 and OptimizeSim3
oracles, one job per task on 16 host threads; the numpy stages hold the interpreter lock, the two oracles do not) with ret, the
correspondences' count and the final matches compared.  `--only chain --no-oracle` is the form a kernel trace is taken of.
No threshold is set on any ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import sim3_opt_cases as sc  # noqa: E402


def measure(fe, cases, a):
    import torch
    off, corr, probs = sc.pack(cases)
    n = len(cases)
    d_c = torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda()
    d_r = torch.zeros(n * sc.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda"); d_s = torch.zeros(len(corr), dtype=torch.uint8, device="cuda")
    L, C = fe.lib(), fe.C
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        fe.check(L.sd_sim3_optimize_device(n, fe._p(off), C.c_void_p(d_c.data_ptr()), fe._p(probs), C.c_void_p(d_r.data_ptr()),
                                           C.c_void_p(d_s.data_ptr()), C.c_void_p(stream)))
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call()
        e1.record(); torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / a.calls)
    res = d_r.cpu().numpy().view(sc.RESULT_DTYPE); st = d_s.cpu().numpy()
    sc.solve_packed(off, corr, probs, sc.WAVE, 16)
    times = {}
    for threads in (1, 16):
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            o_res, o_st, _, _ = sc.solve_packed(off, corr, probs, sc.WAVE, threads)
            ts.append((time.perf_counter() - t) * 1e3)
        times[threads] = sorted(ts)[2]
    same = res.tobytes() == o_res.tobytes() and st.tobytes() == o_st.tobytes()
    return dict(problems=n, correspondences=int(len(corr)), call_ms=round(sorted(runs)[len(runs) // 2], 4), call_ms_runs=[round(x, 4) for x in runs],
                oracle_ms=round(times[16], 3), oracle_threads=16, oracle_ms_one_thread=round(times[1], 3), host_cpus=len(os.sched_getaffinity(0)),
                lm_trials=int(res["trials"].sum()), matched=int((res["ret"] >= 20).sum()), identical_to_oracle=bool(same),
                oracle_over_device=round(times[16] / sorted(runs)[len(runs) // 2], 2))


def bench_chain(pkg, a):
    from concurrent.futures import ThreadPoolExecutor
    import fuse_cases as fc
    import triangulate_cases as tc
    import sim3_refine_cases as rc
    fe, synth = pkg.frontend, pkg.synth
    distinct = 8
    scene = rc.refine_scene(77, a.features, distinct, noise=1.0)
    ws = fc.Workspace(fe, 2 * distinct, tc.vocabulary(synth, 5), dict(W=1241, H=376, nfeatures=2000, scale=1.2, nlevels=8))
    scene["pairs"] = [scene["pairs"][q % distinct] for q in range(a.pairs)]
    timed = []
    got = rc.device_refine(ws, scene, timed=timed)
    call = timed[0]
    for _ in range(a.warmup):
        call()
    ws.b.sync()
    runs = []
    for _ in range(a.runs):
        t = time.perf_counter()
        for _ in range(a.chain_calls):
            call()
        ws.b.sync()
        runs.append((time.perf_counter() - t) * 1e3 / a.chain_calls)
    rec = dict(pairs=a.pairs, distinct_pairs=distinct, features=int(np.mean([len(k["kp"]) for k in scene["kfs"]])),
               correspondences=int(np.mean([g["result"]["n_built"] for g in got])), matched=int(sum(g["result"]["matched"] for g in got)),
               call_ms=round(sorted(runs)[len(runs) // 2], 4), call_ms_runs=[round(x, 4) for x in runs])
    if not a.no_oracle:
        singles = [dict(scene, pairs=[pr]) for pr in scene["pairs"]]
        rc.cpu_refine(singles[0], ws.lv, ws.cap)
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            ref = list(pool.map(lambda s: rc.cpu_refine(s, ws.lv, ws.cap)[0], singles))
        rec["oracle_ms"] = round((time.perf_counter() - t) * 1e3, 1); rec["oracle_threads"] = 16
        rec["identical_decisions"] = bool(all(int(g["result"]["opt"]["ret"]) == r["ret"] and int((g["add12"] >= 0).sum()) == r["added"] for g, r in zip(got, ref)))
        rec["oracle_over_device"] = round(rec["oracle_ms"] / rec["call_ms"], 1)
    ws.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--chain-calls", type=int, default=10)
    ap.add_argument("--only", choices=("chain",), default=None, help="the chain alone (a profiler run); nothing is written")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--correspondences", type=int, default=150)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_opt_bench.json"))
    a = ap.parse_args()
    pkg = g.load_package()
    fe = pkg.frontend
    if fe.device_count() < 1:
        raise SystemExit("bench_sim3_opt needs a HIP device")
    if a.only:
        print(json.dumps({"chain": bench_chain(pkg, a)}))
        return
    n = a.keyframes * a.candidates
    cases = [sc.scene("bench_%d" % k, a.correspondences + (k % 21) - 10, 5000 + k, s=1.0 + 0.01 * (k % 7), fix=k % 2, outliers=a.correspondences // 10,
                      prior=(0.02, 0.1, 0.03)) for k in range(n)]
    rec = dict(tool="bench_sim3_opt", timed_calls=a.calls, batch=measure(fe, cases, a), single=measure(fe, cases[:1], a), chain=bench_chain(pkg, a))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
