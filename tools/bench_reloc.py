"""Timing of the relocalisation matcher and cascade on the device (k_reloc.h), written to profiles/reloc_bench.json and printed as ONE
JSON line.  Workload: `--frames` lost frames x `--candidates` candidate keyframes at about `--features` features a slot (8 distinct
(frame, keyframe) pairs, repeated), of which `--known` are BoW inliers on entry:
  matcher -- ONE sd_batch_search_by_projection_reloc call for all jobs, th = 10, ORBdist = 100
  cascade -- ONE sd_batch_relocalize_refine call for all jobs
Each: a host clock around `--calls` calls that end in the workspace's stream synchronise, after warm-up; the kernels' times from
sd_batch_kernel_times in a pass of their own; the sequential CPU oracle (tests/cpp/reloc_oracle.cpp with pose_oracle.cpp) on the same
work, one job per task on 16 host threads (a task builds the oracle's copy of its own two slots and nothing else), wall clock, median of
three.  The matcher's results are compared byte for byte, the cascade's decisions, final assignment and flags with the free-running
oracle.  No threshold is set on any ratio."""
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
import reloc_cases as rc  # noqa: E402

GEOM = dict(W=1241, H=376, nfeatures=2000, scale=1.2, nlevels=8)
DISTINCT = 8
KERNELS = ("k_reloc_search", "k_reloc_assign", "k_reloc_edges", "k_pose_optimize (reloc)", "k_reloc_begin/after/mark/finish")


def scene(a):
    """DISTINCT (frame, keyframe) pairs: `features` true correspondences spread over the image, `known` of them known on entry (a tenth of
    those wrong), 0.3 px of noise, a PnP-like pose error."""
    rng = np.random.default_rng(77)
    kfs, jobs, pts, pdesc = [], [], [], []
    for q in range(DISTINCT):
        B = rc.Builder(15000 + q)
        held = set(rng.choice(a.features, a.known, replace=False).tolist())
        for i in range(a.features):
            u, v = float(rng.uniform(8, 1225)), float(rng.uniform(8, 365)); z = float(rng.uniform(5, 30))
            p = B.point(tc.from_pixel(rc.I4, u, v, z), 2); B.kf_feature(p, float(rng.choice([0.0, 0.0, 0.0, 20.0, 200.0])))
            off = rng.normal(0, 0.3, 2) + (rng.choice([-25.0, 25.0], 2) if i in held and rng.random() < 0.1 else 0.0)
            f = B.F.add(u + off[0], v + off[1], rc.flipped(B.pdesc[p], int(rng.integers(0, 90)), rng), int(rng.integers(1, 4)), 0.0,
                        stereo_z=z if rng.random() < 0.3 else None)
            if i in held:
                B.held[f] = p
        sc = B.build("bench_%d" % q)
        job = sc["jobs"][0]
        job["frame"], job["kf"] = 2 * q, 2 * q + 1
        job["Tcw"] = tc.pose(tc.rodrigues(rng.normal(0, 0.002, 3)), rng.normal(0, 0.01, 3)).astype(np.float32)
        job["kf_point"] = np.where(job["kf_point"] >= 0, job["kf_point"] + len(pts), -1).astype(np.int32)
        job["frame_point"] = np.where(job["frame_point"] >= 0, job["frame_point"] + len(pts), -1).astype(np.int32)
        job["found"] = None
        kfs += sc["kfs"]; jobs.append(job); pts += list(sc["points"]); pdesc += list(sc["pdesc"])
    return dict(name="bench", kfs=kfs, jobs=jobs, points=np.array(pts, rc.MP_DTYPE), pdesc=np.array(pdesc, np.uint8).reshape(-1, 32))


def timed(ws, call, a):
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
    return round(call_ms, 4), {k: round(kt[k][0] / a.calls, 4) for k in KERNELS if k in kt and kt[k][1]}


def oracle_ms(tasks, fn):
    fn(tasks[0])
    ts, ref = [], None
    for _ in range(3):
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            ref = list(pool.map(fn, tasks))
        ts.append((time.perf_counter() - t) * 1e3)
    return round(sorted(ts)[1], 2), ref


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=5)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--known", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_bench.json"))
    a = ap.parse_args()
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    if fe.device_count() < 1:
        raise SystemExit("bench_reloc needs a HIP device")
    ws = rc.Workspace(fe, 2 * DISTINCT, tc.vocabulary(synth, 5), GEOM)
    try:
        sc = scene(a)
        n_jobs = a.frames * a.candidates
        order = [q % DISTINCT for q in range(n_jobs)]
        jobs = [dict(sc["jobs"][q], th=10.0, orb=100) for q in order]
        got_m = rc.device_search(ws, sc, jobs=jobs)
        got_c = rc.device_refine(ws, sc, upload=False, jobs=jobs)
        kfp = np.full((n_jobs, ws.cap), -1, np.int32); fp = np.full((n_jobs, ws.cap), -1, np.int32)
        for q, j in enumerate(jobs):
            kfp[q, :len(j["kf_point"])] = j["kf_point"]; fp[q, :len(j["frame_point"])] = j["frame_point"]
        d_kfp, d_fp = torch.from_numpy(kfp).cuda(), torch.from_numpy(fp).cuda()
        d_pts = torch.from_numpy(np.frombuffer(sc["points"].tobytes(), np.uint8).copy()).cuda(); d_desc = torch.from_numpy(sc["pdesc"].reshape(-1).copy()).cuda()
        T = np.array([np.asarray(j["Tcw"], np.float32).reshape(16) for j in jobs]); fi = [j["frame"] for j in jobs]; ki = [j["kf"] for j in jobs]
        th = np.full(n_jobs, 10.0, np.float32); orb = np.full(n_jobs, 100, np.int32)
        npts = len(sc["points"])
        m_call = lambda: ws.b.search_by_projection_reloc(fi, ki, T, th, orb, d_kfp.data_ptr(), d_fp.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), tc.CAM, n_points=npts)
        c_call = lambda: ws.b.relocalize_refine(fi, ki, T, d_kfp.data_ptr(), d_fp.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), tc.CAM, n_points=npts)
        m_ms, m_kt = timed(ws, m_call, a)
        c_ms, c_kt = timed(ws, c_call, a)
        one = lambda q: dict(sc, kfs=[sc["kfs"][jobs[q]["frame"]], sc["kfs"][jobs[q]["kf"]]], jobs=[dict(jobs[q], frame=0, kf=1)])
        mo_ms, m_ref = oracle_ms(list(range(n_jobs)), lambda q: rc.cpu_search(one(q), lv=ws.lv)[0][0])
        co_ms, c_ref = oracle_ms(list(range(n_jobs)), lambda q: rc.cpu_refine(one(q), lv=ws.lv)[0])
        m_same = True
        try:
            rc.assert_same(dict(sc, jobs=jobs), got_m, m_ref)
        except AssertionError as e:
            m_same = False; print("matcher differs:", e)
        c_same = all(rc.decisions((x[0], x[1][:len(y[1])], x[2][:len(y[1])])) == rc.decisions(y) for x, y in zip(got_c, c_ref))
        stages = {}
        for x in got_c:
            stages[str(int(x[0]["stage_reached"]))] = stages.get(str(int(x[0]["stage_reached"])), 0) + 1
        rec = dict(tool="bench_reloc", frames=a.frames, candidates=a.candidates, jobs=n_jobs, distinct_pairs=DISTINCT, features=a.features, known_on_entry=a.known,
                   timed_calls=a.calls, host_cpus=len(os.sched_getaffinity(0)),
                   matcher=dict(call_ms=m_ms, kernel_ms=m_kt, oracle_ms=mo_ms, oracle_threads=16, oracle_over_device=round(mo_ms / m_ms, 2),
                                matches=int(sum(x[4] for x in got_m)), identical_to_oracle=bool(m_same)),
                   cascade=dict(call_ms=c_ms, kernel_ms=c_kt, oracle_ms=co_ms, oracle_threads=16, oracle_over_device=round(co_ms / c_ms, 2),
                                stages_reached=stages, matched=int(sum(int(x[0]["matched"]) for x in got_c)), identical_to_oracle=bool(c_same)))
    finally:
        ws.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
