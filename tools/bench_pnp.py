"""Timing of Tracking::Relocalization's PnP stage on the device (k_pnp.h), written to profiles/pnp_bench.json and printed as ONE JSON line.
usage: bench_pnp.py [--frames 64] [--candidates 5] [--matches 100] [--outliers 0.4] [--epsilon 0.2] [--runs 20] [--no-oracle]
Workload: frames x candidates problems of about `matches` BoW matches each (+-20 %), a fraction `outliers` of them wrong, 0.3 px noise,
SetRansacParameters(0.99, 10, 300, 4, epsilon, 5.991).  epsilon = 0.2 makes mRansacMaxIts the full 300; the reference's own 0.5 gives 35,
reported as a second row.  Measured per row:
  device_call_ms      ONE sd_pnp_ransac_device call over all problems, HIP events around it, median of `runs` after 3 warm-up calls
  with_download_ms    the same plus the copy of the records and masks to the host (wall clock around call + synchronise + copy)
  single_problem_ms   one problem alone, the case where a host thread is closest
  oracle_1 / _16      the sequential CPU oracle (tests/cpp/pnp_oracle.cpp, -O2) over the same problems on 1 and 16 host threads, one run;
                      the oracle stops at the first success as the reference does, the device evaluates every iteration 1 .. end
NOT measured here: the chain sd_batch_relocalize_pnp against tools/bench_reloc.py's path with host PnP (this tool times the solver stage,
which needs no frame slots), and the kernel trace, which is taken in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_pnp.py --no-oracle --runs 3).
"""
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
import pnp_cases as pc  # noqa: E402


def workload(a, epsilon):
    rng = np.random.default_rng(2026)
    prs = []
    for k in range(a.frames * a.candidates):
        n = int(a.matches * rng.uniform(0.8, 1.2))
        prs.append(pc.make_problem(1000 + k, n, outliers=a.outliers, noise=0.3, epsilon=epsilon))
    return prs


def device_row(fe, torch, C, prs, kw, runs):
    off, corr, tab = pc.pack(prs)
    n = len(prs)
    L = fe.lib()
    d_c = torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda()
    d_r = torch.zeros(n * pc.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_i = torch.zeros(len(corr), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        fe.check(L.sd_pnp_ransac_device(n, fe._p(off), C.c_void_p(d_c.data_ptr()), fe._p(tab), kw["probability"], kw["min_inliers"], kw["max_iterations"],
                                        kw["min_set"], kw["epsilon"], kw["th2"], C.c_void_p(d_r.data_ptr()), C.c_void_p(d_i.data_ptr()), None, None, 0,
                                        C.c_void_p(stream)))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        call(); torch.cuda.synchronize(); res = d_r.cpu().numpy(); inl = d_i.cpu().numpy()
        wall.append((time.perf_counter() - t0) * 1e3)
    res = res.view(pc.RESULT_DTYPE)
    return dict(device_call_ms=round(float(np.median(ev)), 4), device_call_min_ms=round(float(np.min(ev)), 4), with_download_ms=round(float(np.median(wall)), 4),
                kinds={str(k): int((res["kind"] == k).sum()) for k in (0, 1, 2)}, iterations_evaluated=int(sum(pc.end_of(p, r) for p, r in zip(prs, res))),
                refines=int(res["n_refines"].sum())), (off, corr, tab, res, inl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64); ap.add_argument("--candidates", type=int, default=5)
    ap.add_argument("--matches", type=int, default=100); ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--epsilon", type=float, default=0.2); ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    import ctypes as C
    import torch
    fe = g.load_package().frontend
    if fe.device_count() < 1:
        raise SystemExit("bench_pnp needs a HIP device")
    rec = dict(tool="bench_pnp", problems=a.frames * a.candidates, matches=a.matches, outliers=a.outliers, runs=a.runs, rows=[])
    for eps in (a.epsilon, 0.5):
        prs = workload(a, eps)
        kw = pc.params_of(prs[0])
        row, (off, corr, tab, res, inl) = device_row(fe, torch, C, prs, kw, a.runs)
        row.update(epsilon=eps, max_its=int(res["max_its"].max()), correspondences=int(len(corr)))
        one, _ = device_row(fe, torch, C, prs[:1], kw, a.runs)
        row["single_problem_ms"] = one["device_call_ms"]; row["single_problem_with_download_ms"] = one["with_download_ms"]
        if not a.no_oracle:
            pc.oracle()                                                   # built before the clock starts
            for th in (1, 16):
                t0 = time.perf_counter()
                o_res, o_inl = pc.iterate_packed(off, corr, tab, kw, order=1, threads=th)
                row["oracle_%d_threads_ms" % th] = round((time.perf_counter() - t0) * 1e3, 3)
            row["oracle_iterations_run"] = int(o_res["iteration"].sum())
            row["equals_oracle"] = bool(o_res.tobytes() == res.tobytes() and o_inl.tobytes() == inl.tobytes())
            t0 = time.perf_counter()
            pc.iterate_packed(off[:2], corr[:off[1]], tab[:1], kw, order=1, threads=1)
            row["oracle_single_problem_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        rec["rows"].append(row)
    rec["not_measured"] = ["the chain against tools/bench_reloc.py's path with host PnP (sd_batch_relocalize_pnp; this tool times the solver stage alone)",
                           "bench.py's headline (its path is untouched)"]
    if not a.no_oracle:
        with open(os.path.join(ROOT, "profiles", "pnp_bench.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
