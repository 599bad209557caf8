"""Timing of LocalMapping::SearchInNeighbors' matcher on the device (k_fuse.h), written to profiles/fuse_bench.json and printed as ONE
JSON line.  A camera moves 0.7 m per keyframe through a cloud of points; every feature of a keyframe observes a world point and 30 % hold it
as their map point already.
  forward      -- the first loop: `--keyframes` keyframes, each fusing its ~`--features` points into its `--targets` next keyframes: ONE
                  sd_batch_fuse call of keyframes x targets jobs (entries of points the target already holds are -1); a host clock around
                  `--calls` calls after warm-up that ends in the workspace's stream synchronise, per call, and the two kernels' times from
                  sd_batch_kernel_times in a pass of their own; the sequential CPU oracle (tests/cpp/fuse_oracle.cpp) on the same jobs over 16
                  host threads, wall clock; results compared byte for byte.
  reverse      -- the second loop: per keyframe one job of targets x features candidates (the targets' points) into the keyframe.
  per_candidate -- from sd_batch_kernel_times of the same run: k_fuse_search and k_local_candidates on the same frames, points and window
                  size (Fuse with th = 4, SearchLocalPoints with th = 1 and view cosines below 0.998: both radii are 4 * scale[level]),
                  nanoseconds per candidate.  No threshold is set on either."""
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

GEOM = dict(W=1241, H=376, nfeatures=2000, scale=1.2, nlevels=8)


def world(n_kf, n_feat, seed=3):
    """-> (keyframes [dict + `point`: world point of every feature], points MP_DTYPE, descriptors).  Vectorised."""
    rng = np.random.default_rng(seed)
    lv = tc.Levels()
    n_pts = 40 * n_kf + 8000
    Xw = np.stack([rng.uniform(-25, 25, n_pts), rng.uniform(-6, 6, n_pts), rng.uniform(2, 0.7 * n_kf + 70, n_pts)], 1)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)

    def flips(n, kmax):
        k = rng.integers(0, kmax + 1, n)
        m = np.zeros((n, 256), np.uint8)
        pos = rng.integers(0, 256, (n, kmax))
        for j in range(kmax):
            m[np.arange(n), pos[:, j]] |= (j < k).astype(np.uint8)
        return np.packbits(m, axis=1, bitorder="little")

    pts = np.zeros(n_pts, fc.MP_DTYPE)
    pts["xw"] = Xw
    tilt = np.array([0.17, 0.0, 1.0]) / np.linalg.norm([0.17, 0.0, 1.0])          # 10 degrees off the path: view cosines below 0.998
    pts["normal"] = tilt
    pts["flags"] = 1
    first_dist = np.full(n_pts, np.nan)
    cam = tc.CAM
    out = []
    for k in range(n_kf):
        T = tc.pose(tc.rodrigues(rng.normal(size=3) * 0.02), [0, 0, 0]) @ tc.pose(np.eye(3), [-0.15 * np.sin(0.3 * k), 0.0, -0.7 * k])
        Xc = Xw @ T[:3, :3].T + T[:3, 3]
        z = Xc[:, 2]
        u = float(cam["fx"]) * Xc[:, 0] / z + float(cam["cx"]); v = float(cam["fy"]) * Xc[:, 1] / z + float(cam["cy"])
        vis = np.nonzero((z > 3) & (z < 60) & (u > 0) & (u < 1241) & (v > 0) & (v < 376))[0]
        vis = rng.permutation(vis)[:n_feat]
        n = len(vis)
        dist = np.linalg.norm(Xc[vis], axis=1)
        new = np.isnan(first_dist[vis])
        first_dist[vis[new]] = dist[new] * 1.2 ** rng.integers(0, 6, int(new.sum()))       # mfMaxDistance: the level it was created at
        level = np.clip(np.ceil(np.log(first_dist[vis] / dist) / np.log(1.2)), 0, 7).astype(np.int32)
        octave = np.clip(level - rng.integers(0, 2, n), 0, 7)
        s = lv.scale[octave]
        kp = np.zeros(n, tc.KP_DTYPE)
        kp["x"] = u[vis] + rng.normal(size=n) * 0.5 * s; kp["y"] = v[vis] + rng.normal(size=n) * 0.5 * s
        kp["size"] = 31 * s; kp["angle"] = rng.uniform(0, 360, n); kp["response"] = 50; kp["octave"] = octave; kp["class_id"] = -1
        stereo = rng.random(n) < 0.7
        depth = np.where(stereo, z[vis] * (1 + rng.normal(size=n) * 0.003), -1).astype(np.float32)
        ur = np.where(stereo, kp["x"] - cam["mbf"] / np.where(stereo, depth, 1), -1).astype(np.float32)
        out.append(dict(kp=kp, desc=base[vis] ^ flips(n, 40), ur=ur, depth=depth, Tcw=T.astype(np.float32), point=vis.astype(np.int32),
                        holds=rng.random(n) < 0.3))
    first_dist[np.isnan(first_dist)] = 30.0
    pts["max_distance"] = first_dist
    pts["min_distance"] = first_dist / float(lv.scale[-1])
    return out, pts, base


def jobs_of(kfs, n_kf, n_targets):
    """-> (forward jobs, reverse jobs): (target slot, entries, state)"""
    fwd, rev = [], []
    for k in range(n_kf):
        back = []
        for t in range(k + 1, k + 1 + n_targets):
            held = set(kfs[t]["point"][kfs[t]["holds"]].tolist())
            e = kfs[k]["point"].copy()
            e[np.isin(e, list(held))] = -1                                     # IsInKeyFrame(target)
            fwd.append((t, e, kfs[t]["holds"].astype(np.uint8)))
            back.append(kfs[t]["point"])
        e = np.unique(np.concatenate(back))                                    # the targets' points, each once
        e = e[~np.isin(e, kfs[k]["point"][kfs[k]["holds"]])]                 # IsInKeyFrame(keyframe)
        rev.append((k, e.astype(np.int32), kfs[k]["holds"].astype(np.uint8)))
    return fwd, rev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.json"))
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    if fe.device_count() < 1:
        raise SystemExit("bench_fuse needs a HIP device")
    n_kf, nt = a.keyframes, a.targets
    kfs, pts, pdesc = world(n_kf + nt, a.features)
    ws = fc.Workspace(fe, n_kf + nt, tc.vocabulary(synth, 5), GEOM)
    ws.upload_grid(kfs)
    fwd, rev = jobs_of(kfs, n_kf, nt)
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda()
    d_desc = torch.from_numpy(pdesc.reshape(-1).copy()).cuda()
    stream = None                                            # the workspace's own stream
    rec = dict(tool="bench_fuse", keyframes=n_kf, targets=nt, features=int(np.mean([len(k["kp"]) for k in kfs])), timed_calls=a.calls)
    L = fc.oracle()
    okfs = [fc.OracleKF(L, k, lv=ws.lv) for k in kfs]
    for name, jobs in (("forward", fwd), ("reverse", rev)):
        off = np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int32)
        d_ent = torch.from_numpy(np.concatenate([j[1] for j in jobs]).astype(np.int32)).cuda()
        st = np.zeros((len(jobs), ws.cap), np.uint8)
        for q, j in enumerate(jobs):
            st[q, :len(j[2])] = j[2]
        d_st = torch.from_numpy(st).cuda()
        slots = np.array([j[0] for j in jobs], np.int32); T = np.stack([kfs[j[0]]["Tcw"] for j in jobs])

        def call(th=3.0):
            ws.b.fuse(slots, T, off, d_ent.data_ptr(), d_pts.data_ptr(), d_desc.data_ptr(), tc.CAM, th=th, d_kf_state=d_st.data_ptr(),
                      stream=stream, n_points=len(pts))
        for _ in range(a.warmup):
            call()
        ws.b.sync()
        t = time.perf_counter()                              # the library runs on its own stream: a host clock around work that ends in its sync
        for _ in range(a.calls):
            call()
        ws.b.sync()
        call_ms = (time.perf_counter() - t) * 1e3 / a.calls
        ws.b.set_profiling(True); ws.b.reset_kernel_times()  # kernel times in a pass of their own
        for _ in range(a.calls):
            call()
        ws.b.sync()
        kt = ws.b.kernel_times()
        ws.b.set_profiling(False)
        got = [ws.b.download_fuse(q) for q in range(len(jobs))]
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            ref = list(pool.map(lambda j: fc.run_job(L, okfs[j[0]], j[1], pts, pdesc, j[2], 3.0), jobs))
        oracle_ms = (time.perf_counter() - t) * 1e3
        same = all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2] for x, y in zip(got, ref))
        rec[name] = dict(jobs=len(jobs), entries=int(off[-1]), fused=int(sum(x[2] for x in got)), call_ms=round(call_ms, 4),
                         kernel_ms={k: round(kt[k][0] / max(kt[k][1], 1), 4) for k in ("k_fuse_search", "k_fuse_resolve")}, oracle_ms=round(oracle_ms, 2), oracle_threads=16, identical_to_oracle=bool(same))
    # ---- per candidate: k_fuse_search beside k_local_candidates, same frames, points and window size
    nf = min(len(fwd), n_kf + nt)                                  # sd_batch_search_local_map takes at most max_images frames
    sel = fwd[:nf]
    gathered = [j[1][j[1] >= 0] for j in sel]
    off = np.concatenate([[0], np.cumsum([len(x) for x in gathered])]).astype(np.int32)
    idx = np.concatenate(gathered)
    total = int(off[-1])
    g_pts = torch.from_numpy(np.frombuffer(pts[idx].tobytes(), np.uint8).copy()).cuda()
    g_desc = torch.from_numpy(pdesc[idx].reshape(-1).copy()).cuda()
    ident = torch.arange(total, dtype=torch.int32).cuda()
    slots = np.array([j[0] for j in sel], np.int32); T = np.stack([kfs[j[0]]["Tcw"] for j in sel])
    track = torch.zeros(total * 24, dtype=torch.uint8).cuda(); pm = torch.zeros(total, dtype=torch.int32).cuda()
    km = torch.zeros(nf * ws.cap, dtype=torch.int32).cuda(); nm = torch.zeros(nf, dtype=torch.int32).cuda()
    ws.b.set_profiling(True)
    for rep in range(a.warmup + 10 * a.calls):
        if rep == a.warmup:
            ws.b.sync(); ws.b.reset_kernel_times()
        ws.b.fuse(slots, T, off, ident.data_ptr(), g_pts.data_ptr(), g_desc.data_ptr(), tc.CAM, th=4.0, stream=stream, n_points=total)
        ws.b.search_local_map(slots, off, g_pts.data_ptr(), g_desc.data_ptr(), T, tc.CAM, 1.0, 0.8, track.data_ptr(), pm.data_ptr(), km.data_ptr(),
                              nm.data_ptr(), stream=stream)
    ws.b.sync()
    kt = ws.b.kernel_times()
    ws.b.set_profiling(False)
    rec["per_candidate"] = dict(frames=nf, candidates=total, window="4 * scale[level]",
                                **{k: dict(ms_per_call=round(kt[k][0] / max(kt[k][1], 1), 4), ns_per_candidate=round(kt[k][0] / max(kt[k][1], 1) * 1e6 / total, 2))
                                   for k in ("k_fuse_search", "k_fuse_resolve", "k_local_candidates", "k_local_resolve")})
    for o in okfs:
        o.close()
    ws.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
