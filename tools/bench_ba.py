"""Timing of Optimizer::LocalBundleAdjustment on the device (k_ba.h), written to profiles/ba_bench.json and printed as ONE JSON line.
`--problems` problems (default 64) of `--local` + `--fixed` keyframes (30 + 20), `--points` points (1,500), each seen by 8 keyframes (about
12 k edges), 1 px noise, 3 % gross outliers, in ONE sd_local_ba_device call on device arrays:
  device_ms  -- a host clock around `--calls` calls after warm-up, ended by a stream synchronise, per call
  oracle_ms  -- the sequential CPU oracle (tests/cpp/ba_oracle.cpp) on the same problems over 16 host threads, wall clock, same machine
  phases_ms  -- with --profile (default on): one more call with the library's profiling switch on (sd_local_ba_set_profiling), in a pass of its
                own; the device wall-clock time per phase, mean and maximum over the problems, and the slowest problem's own breakdown
  identical_decisions -- erase / level-1 flags and the iteration, trial and rejection counts of every problem equal the oracle's
No threshold is set on either number."""
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
import ba_cases as bc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--local", type=int, default=30)
    ap.add_argument("--fixed", type=int, default=20)
    ap.add_argument("--points", type=int, default=1500)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_bench.json"))
    a = ap.parse_args()
    import torch
    fe = g.load_package().frontend
    if fe.device_count() < 1:
        raise SystemExit("bench_ba needs a HIP device")
    probs = [bc.problem_of(bc.make_scene(7000 + q, a.local, a.fixed, a.points, stereo_frac=0.7, noise=1.0, obs_per_point=a.views, mild=0.03))
             for q in range(a.problems)]
    ko, nl, po, eo, kfs, xw, ed, ref = fe.pack_ba_problems(probs)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d_in = [dev(kfs), dev(xw), dev(ed), dev(ref)]
    outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (len(kfs) * 64, len(xw) * 12, len(xw) * 12, len(xw) * 4, len(ed), len(ed), a.problems * 48)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    stream = torch.cuda.Stream()

    def call():
        fe.check(fe.lib().sd_local_ba_device(a.problems, p(ko), p(nl), p(po), p(eo), *[C.c_void_p(t.data_ptr()) for t in d_in + outs],
                                             C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        call()
    stream.synchronize()
    t = time.perf_counter()
    for _ in range(a.calls):
        call()
    stream.synchronize()
    device_ms = (time.perf_counter() - t) * 1e3 / a.calls
    phases = None
    if a.profile:
        fe.local_ba_profile(a.problems, on=True)
        call()
        ms = fe.local_ba_profile(a.problems)
        fe.local_ba_profile(a.problems, on=False)
        slow = int(ms.sum(1).argmax())
        phases = dict(mean={k: round(float(v), 3) for k, v in zip(fe.BA_PHASES, ms.mean(0))},
                      max={k: round(float(v), 3) for k, v in zip(fe.BA_PHASES, ms.max(0))},
                      slowest_problem=dict(index=slow, **{k: round(float(v), 3) for k, v in zip(fe.BA_PHASES, ms[slow])}),
                      per_problem_total_ms=[round(float(v), 2) for v in ms.sum(1)])
    l1, er, st = outs[4].cpu().numpy(), outs[5].cpu().numpy(), outs[6].cpu().numpy().view(fe.BA_STATS_DTYPE)
    bc.oracle()
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        want = list(pool.map(bc.run_oracle_plain, probs))
    oracle_ms = (time.perf_counter() - t) * 1e3
    same = all(np.array_equal(l1[eo[q]:eo[q + 1]], w["level1"]) and np.array_equal(er[eo[q]:eo[q + 1]], w["erase"]) and
               all(np.array_equal(st[q][f], w["stats"][f]) for f in bc.COUNTS) for q, w in enumerate(want))
    rec = dict(tool="bench_ba", problems=a.problems, local_keyframes=a.local, fixed_keyframes=a.fixed, points=a.points,
               edges_per_problem=int(len(ed) / a.problems), timed_calls=a.calls, device_ms=round(device_ms, 2),
               device_ms_per_problem=round(device_ms / a.problems, 3), oracle_ms=round(oracle_ms, 1), oracle_threads=16,
               phases_ms=phases, lm_trials_per_problem=round(float(st["trials"].sum()) / a.problems, 1), identical_decisions=bool(same))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
