"""Timing of the loop-closing matchers on the device (k_loop.h), written to profiles/loop_bench.json and printed as ONE JSON line.
  bow     -- `--pairs` SearchByBoW(pKF1, pKF2) pairs at about `--features` features a keyframe (8 distinct pairs, repeated): ONE
             sd_batch_search_by_bow_kf call
  project -- `--proj-jobs` SearchByProjection(pKF, Scw, ...) jobs of `--candidates` candidates over 8 distinct keyframes, th = 10
  fuse    -- `--fuse-jobs` Fuse(pKF, Scw, ...) jobs of `--candidates` candidates over the same keyframes, th = 4
Each: a host clock around `--calls` calls that end in the workspace's stream synchronise, after warm-up; the kernels' times from
sd_batch_kernel_times in a pass of their own; the sequential CPU oracle (tests/cpp/loop_oracle.cpp) on the same work, one job or pair per
task on 16 host threads (a task builds the oracle's copy of its own keyframe, or of its two, and nothing else), wall clock, median of
three; results compared byte for byte.  No threshold is set on any ratio: the assignment
phase of the projection is serial per job, and one job need not beat the host."""
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
import loop_cases as lc  # noqa: E402

GEOM = dict(W=1241, H=376, nfeatures=2000, scale=1.2, nlevels=8)
DISTINCT = 8


def timed(ws, call, a, kernels):
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
    return round(call_ms, 4), {k: round(kt[k][0] / max(kt[k][1], 1), 4) for k in kernels}


def oracle_ms(tasks, fn):
    fn(tasks[0])
    ts, ref = [], None
    for _ in range(3):
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            ref = list(pool.map(fn, tasks))
        ts.append((time.perf_counter() - t) * 1e3)
    return round(sorted(ts)[1], 2), ref


def scw_scene(a, n_jobs):
    sc = fc.random_scene(91, DISTINCT, a.candidates, n_features=a.features, noise=1.5)
    sc = lc.with_scale(sc, 1.37)
    rows = lc.matched_from_state(sc)
    order = [q % DISTINCT for q in range(n_jobs)]
    sc["jobs"] = [sc["jobs"][q] for q in order]; sc["scw"] = [sc["scw"][q] for q in order]; sc["matched"] = [rows[q] for q in order]
    sc["th"] = 4.0; sc["th_proj"] = 10
    return sc


def bench_scw(ws, a, which):
    import torch
    n_jobs = a.proj_jobs if which == "project" else a.fuse_jobs
    sc = scw_scene(a, n_jobs)
    got = (lc.device_project if which == "project" else lc.device_fuse)(ws, sc)
    jobs = sc["jobs"]
    off, d_ent, d_pts, d_desc, S, npts = lc._tables(sc)
    kf = [j[0] for j in jobs]
    if which == "project":
        m = np.full((n_jobs, ws.cap), -1, np.int32)
        for q, row in enumerate(sc["matched"]):
            m[q, :len(row)] = row
        d_m = torch.from_numpy(m).cuda()
        call = lambda: ws.b.search_by_projection_sim3(kf, S, off, d_ent.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), d_m.data_ptr(), tc.CAM,
                                                      th=10, n_points=npts)
        kernels = ("k_loop_search<1>", "k_loop_assign")
        one = lambda q: lc.cpu_project(dict(sc, kfs=[sc["kfs"][jobs[q][0]]], jobs=[(0,) + tuple(jobs[q][1:])], scw=[sc["scw"][q]],
                                            matched=[sc["matched"][q]]), lv=ws.lv, cap=ws.cap)[0][0]
        same = lambda x, y: x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2]
    else:
        st = np.zeros((n_jobs, ws.cap), np.uint8)
        for q, j in enumerate(jobs):
            st[q, :len(j[2])] = j[2]
        d_m = torch.from_numpy(st).cuda()
        call = lambda: ws.b.fuse_sim3(kf, S, off, d_ent.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), tc.CAM, th=4.0, d_kf_state=d_m.data_ptr(),
                                      n_points=npts)
        kernels = ("k_loop_search<0>", "k_fuse_resolve")
        one = lambda q: lc.cpu_fuse(dict(sc, kfs=[sc["kfs"][jobs[q][0]]], jobs=[(0,) + tuple(jobs[q][1:])], scw=[sc["scw"][q]]), lv=ws.lv)[0][0]
        same = lambda x, y: x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2]
    call_ms, kt = timed(ws, call, a, kernels)
    o_ms, ref = oracle_ms(list(range(n_jobs)), one)
    return dict(jobs=n_jobs, candidates=a.candidates, features=int(np.mean([len(k["kp"]) for k in sc["kfs"]])), matched=int(sum(x[2] for x in got)),
                call_ms=call_ms, kernel_ms=kt, oracle_ms=o_ms, oracle_threads=16, identical_to_oracle=bool(all(same(x, y) for x, y in zip(got, ref))))


def bench_bow(ws, orc, voc, a):
    import torch
    O = orc.Vocabulary.from_nodes(voc)
    sc = fc.random_scene(92, 2 * DISTINCT, int(a.features * 1.25), n_features=a.features, noise=0.5)
    kfs = sc["kfs"]
    tc.attach_bow(kfs, O)
    ws.upload(kfs)
    rng = np.random.default_rng(5)
    cases = [dict(kf1=kfs[2 * q], kf2=kfs[2 * q + 1], nnratio=0.75, check_orientation=True,
                  valid1=(rng.random(len(kfs[2 * q]["kp"])) < 0.9).astype(np.uint8), valid2=(rng.random(len(kfs[2 * q + 1]["kp"])) < 0.9).astype(np.uint8))
             for q in range(DISTINCT)]
    order = [q % DISTINCT for q in range(a.pairs)]
    v1 = np.zeros((a.pairs, ws.cap), np.uint8); v2 = np.zeros((a.pairs, ws.cap), np.uint8)
    for p, q in enumerate(order):
        v1[p, :len(cases[q]["valid1"])] = cases[q]["valid1"]; v2[p, :len(cases[q]["valid2"])] = cases[q]["valid2"]
    d1, d2 = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    k1 = [2 * q for q in order]; k2 = [2 * q + 1 for q in order]
    call = lambda: ws.b.search_by_bow_kf(k1, k2, 0.75, True, d1.data_ptr(), d2.data_ptr())
    call()
    got = []
    for p, q in enumerate(order):
        m, _, nm = ws.b.download_matches(p)
        got.append((m[:len(cases[q]["kf1"]["kp"])].copy(), nm))
    call_ms, kt = timed(ws, call, a, ("k_search_by_bow_kf",))
    o_ms, ref = oracle_ms(order, lambda q: lc.cpu_bow(cases[q])[:2])
    same = all(x[0].tobytes() == y[0].tobytes() and x[1] == y[1] for x, y in zip(got, ref))
    return dict(pairs=a.pairs, distinct_pairs=DISTINCT, features=int(np.mean([len(k["kp"]) for k in kfs])), matches=int(sum(x[1] for x in got)),
                call_ms=call_ms, kernel_ms=kt, oracle_ms=o_ms, oracle_threads=16, identical_to_oracle=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--proj-jobs", type=int, default=16)
    ap.add_argument("--fuse-jobs", type=int, default=30)
    ap.add_argument("--candidates", type=int, default=4000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_bench.json"))
    a = ap.parse_args()
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    if fe.device_count() < 1:
        raise SystemExit("bench_loop needs a HIP device")
    voc = synth.vocabulary(k=10, L=4, seed=5, early_leaf_frac=0.0, stop_frac=0.0)       # FeatureVector nodes at level 2: about 20 features each
    ws = lc.Workspace(fe, max(a.pairs, 2 * DISTINCT), voc, GEOM)
    try:
        rec = dict(tool="bench_loop", timed_calls=a.calls, host_cpus=len(os.sched_getaffinity(0)), bow=bench_bow(ws, g.load_oracle(), voc, a),
                   project=bench_scw(ws, a, "project"), fuse=bench_scw(ws, a, "fuse"))
    finally:
        ws.close()
    for k in ("bow", "project", "fuse"):
        rec[k]["oracle_over_device"] = round(rec[k]["oracle_ms"] / rec[k]["call_ms"], 2)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
