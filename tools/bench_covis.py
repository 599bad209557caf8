"""Timing of the device covisibility graph (k_covis.h), written to profiles/covis_bench.json and printed as ONE JSON line.
A map of `--keyframes` keyframes x `--features` features with about `--matched` of them matched: a point is seen by six of twelve
neighbouring keyframe ids.  Measured: the rebuild of the index by map point, UpdateConnections for 1 and 64 keyframes, one KeyFrameCulling
call over 100 candidates, UpdateLocalKeyFrames + UpdateLocalPoints for 1 and 64 frames.  Per item
  device_ms   a host clock around a call and the download that synchronises, median of `--calls` after warm-up
  oracle_ms   the sequential CPU oracle (tests/cpp/covis_oracle.cpp) on the same input on 1 host thread, median of three; the local map,
              which only reads, also spread over 16 host threads (UpdateConnections writes and the culling loop is sequential: 1 thread)
Results are compared inside the run.  No ratio is required."""
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
import covis_cases as cc  # noqa: E402


def median(fn, n):
    ts, out = [], None
    for _ in range(n):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=4096)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--matched", type=float, default=0.3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_bench.json"))
    a = ap.parse_args()
    fe = g.load_package().frontend
    if fe.device_count() < 1:
        raise SystemExit("bench_covis needs a HIP device")
    rng = np.random.default_rng(7)
    N, F = a.keyframes, a.features
    P = int(N * F * a.matched / 6)
    centre = rng.integers(0, N, P)
    off = np.argsort(rng.random((P, 12)), axis=1)[:, :6]
    kf = ((centre[:, None] + off) % N).reshape(-1).astype(np.int32)
    pt = np.repeat(np.arange(P, dtype=np.int32), 6)
    order = np.argsort(kf, kind="stable")
    kf, pt = kf[order], pt[order]
    first = np.searchsorted(kf, np.arange(N))
    idx = (np.arange(len(kf)) - first[kf]).astype(np.int32)
    keep = idx < F
    kf, pt, idx = kf[keep], pt[keep], idx[keep]
    octave = rng.choice([0, 1, 2, 3], (N, F), p=[0.6, 0.25, 0.1, 0.05]).astype(np.uint8)
    uright = np.where(rng.random((N, F)) < 0.5, 3.0, -1.0).astype(np.float32)
    depth = rng.choice([1.0, 50.0], (N, F), p=[0.9, 0.1]).astype(np.float32)
    dev = fe.CovisibilityGraph(N, N * F, P, 100, 1 << 16)
    orc = cc.OracleGraph(N)
    L = orc.L
    rec = dict(tool="bench_covis", keyframes=N, features=F, points=P, matches=int(len(kf)), timed_calls=a.calls, host_cpus=len(os.sched_getaffinity(0)), items={})
    try:
        for k in range(N):
            dev.add_host(k, octave[k], uright[k], depth[k], k == 0)
            assert L.sd_covis_oracle_add(orc.h, k, F, cc._p(octave[k]), cc._p(uright[k]), cc._p(depth[k]), int(k == 0)) == 0
        dev.set_matches(kf, idx, pt)
        for k, i, p in zip(kf.tolist(), idx.tolist(), pt.tolist()):
            L.sd_covis_oracle_set_match(orc.h, k, i, p)
        ids64 = [int(x) for x in rng.permutation(N)[:64]]
        # everything connected once, so that the timed calls are the steady state (AddConnection finds its weight in place)
        for base in range(0, N, 100):
            dev.update_connections(list(range(base, min(base + 100, N))))
        for k in range(N):
            L.sd_covis_oracle_update(orc.h, k)
        same = True

        def touch():                                             # a match rewritten with its own value: the index is stale again
            dev.set_matches(kf[:1], idx[:1], pt[:1])

        def dev_update(ids, stale):
            def run():
                if stale:
                    touch()
                dev.update_connections(ids); return dev.connections(ids[0])
            return run

        t_clean, _ = median(dev_update(ids64[:1], False), a.calls)
        t_stale, _ = median(dev_update(ids64[:1], True), a.calls)
        rec["items"]["index_rebuild"] = dict(device_ms=round(t_stale - t_clean, 4), note="update_connections of 1 keyframe after a match changed, minus the same with the index in place")
        for n in (1, 64):
            ids = ids64[:n]
            td, _ = median(dev_update(ids, False), a.calls)
            to, _ = median(lambda: [L.sd_covis_oracle_update(orc.h, k) for k in ids], 3)
            ok = all(cc.device_conn(dev, k) == orc.connections(k) for k in ids)
            same &= ok
            rec["items"]["update_connections_%d" % n] = dict(device_ms=td, oracle_ms_1_thread=to, identical_to_oracle=bool(ok))
        cand = [int(x) for x in dev.connections(ids64[0])["ordered_id"]]
        more = [int(x) for x in rng.permutation(N) if int(x) not in cand and int(x) != 0]
        cand = (cand + more)[:100]
        td, got = median(lambda: dev.keyframe_culling(cand, None, False, 40.0), a.calls)
        clones = [orc.clone() for _ in range(3)]
        it = iter(clones)
        to, ref = median(lambda: next(it).culling(cand, None, False, 40.0, in_place=True), 3)
        for c in clones:
            c.close()
        ok = cc.cull_record([(x["flag"], x["n_mps"], x["n_redundant"]) for x in got]) == ref
        same &= ok
        rec["items"]["keyframe_culling_100"] = dict(device_ms=td, oracle_ms_1_thread=to, identical_to_oracle=bool(ok), flagged=int(sum(x[0] for x in ref[1])))
        frames = []
        for _ in range(64):
            k = int(rng.integers(0, N))
            mine = pt[kf == k]
            frames.append(np.where(rng.random(F) < 0.25, rng.choice(mine, F), -1).astype(np.int32))
        for n in (1, 64):
            fr = frames[:n]
            td, got = median(lambda: dev.local_map(fr), max(a.calls // 4, 3))
            to, ref = median(lambda: [orc.local_map(f, P) for f in fr], 3)
            with ThreadPoolExecutor(16) as pool:
                to16, ref16 = median(lambda: list(pool.map(lambda f: orc.local_map(f, P), fr)), 3)
            dg = [cc.local_record(x["local_kf"], x["reference_kf"], x["local_points"], x["info"]["n_voted"], x["entry_bad"]) for x in got]
            ok = dg == ref and ref16 == ref
            same &= ok
            rec["items"]["local_map_%d" % n] = dict(device_ms=td, oracle_ms_1_thread=to, oracle_ms_16_threads=to16, identical_to_oracle=bool(ok),
                                                    local_keyframes=int(np.mean([len(r[1]) for r in ref])), local_points=int(np.mean([len(r[3]) for r in ref])))
        for v in rec["items"].values():
            if "oracle_ms_1_thread" in v:
                v["oracle_1_thread_over_device"] = round(v["oracle_ms_1_thread"] / v["device_ms"], 2)
        rec["identical_to_oracle"] = bool(same)
    finally:
        dev.close(); orc.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    sys.exit(0 if rec.get("identical_to_oracle") else 1)


if __name__ == "__main__":
    main()
