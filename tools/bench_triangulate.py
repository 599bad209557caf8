"""Timing of LocalMapping::CreateNewMapPoints on the device (k_triangulate.h), printed as ONE JSON line:
  call_ms     -- one sd_batch_create_new_map_points call for `--keyframes` keyframes x `--neighbours` neighbours at `--features` features
                 (a camera moving 0.7 m per keyframe through a cloud of points; keyframe k's neighbours are the next ones along the
                 path; 70 % stereo points, 30 % of the features already hold a map point; FeatureVector nodes of about 20 features),
                 device events around `--calls` calls after warm-up, per call;
  oracle_ms   -- the sequential CPU oracle (tests/cpp/triangulate_oracle.cpp) on the same keyframes over 16 host threads, wall clock;
  new_points  -- map points created per call (device and oracle agree, checked).
--call-only runs just the calls (for `rocprofv3 --kernel-trace --stats -- python tools/bench_triangulate.py --call-only`)."""
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

LEVELSUP = 1            # level-2 nodes of the k = 10, L = 3 vocabulary: 100 nodes, about 20 of 2,000 features each
GEOM = dict(W=1241, H=376, nfeatures=2000, scale=1.2, nlevels=8)


def keyframes(voc, n_kf, n_feat, seed=3):
    """n_kf keyframes along a path, vectorised.  A world point's descriptor is a level-2 node's with 30 bits flipped; an observation
    flips up to 40 more."""
    rng = np.random.default_rng(seed)
    lv = tc.Levels()
    level1 = np.nonzero(voc["parent"] == 0)[0] + 1
    level2 = np.nonzero(np.isin(voc["parent"], level1))[0]
    n_pts = 40 * n_kf + 8000
    Xw = np.stack([rng.uniform(-25, 25, n_pts), rng.uniform(-6, 6, n_pts), rng.uniform(2, 0.7 * n_kf + 70, n_pts)], 1)

    def flips(n, kmax):
        """n random 256-bit masks of 0..kmax set bits"""
        k = rng.integers(0, kmax + 1, n)
        m = np.zeros((n, 256), np.uint8)
        pos = rng.integers(0, 256, (n, kmax))
        for j in range(kmax):
            m[np.arange(n), pos[:, j]] |= (j < k).astype(np.uint8)
        return np.packbits(m, axis=1, bitorder="little")

    base = voc["desc"][rng.choice(level2, n_pts)] ^ flips(n_pts, 30)
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
        octave = rng.integers(0, 8, n)
        s = lv.scale[octave]
        kp = np.zeros(n, tc.KP_DTYPE)
        kp["x"] = u[vis] + rng.normal(size=n) * 0.5 * s; kp["y"] = v[vis] + rng.normal(size=n) * 0.5 * s
        kp["size"] = 31 * s; kp["angle"] = rng.uniform(0, 360, n); kp["response"] = 50; kp["octave"] = octave; kp["class_id"] = -1
        stereo = rng.random(n) < 0.7
        depth = np.where(stereo, z[vis] * (1 + rng.normal(size=n) * 0.01), -1).astype(np.float32)
        ur = np.where(stereo, kp["x"] - cam["mbf"] / np.where(stereo, depth, 1), -1).astype(np.float32)
        out.append(dict(kp=kp, desc=base[vis] ^ flips(n, 40), ur=ur, depth=depth, Tcw=T.astype(np.float32), has_mp=(rng.random(n) < 0.3).astype(np.uint8)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=256)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--call-only", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    if fe.device_count() < 1:
        raise SystemExit("bench_triangulate needs a HIP device")
    voc = tc.vocabulary(synth, 5)
    n_kf, nn = a.keyframes, a.neighbours
    kfs = keyframes(voc, n_kf + nn, a.features)
    ws = tc.Workspace(fe, n_kf + nn, voc, GEOM)
    ws.upload(kfs, levelsup=LEVELSUP)
    off = np.arange(n_kf + 1, dtype=np.int32) * nn
    nb = np.concatenate([np.arange(k + 1, k + 1 + nn) for k in range(n_kf)]).astype(np.int32)
    hk = ws.has_table(kfs[:n_kf]); hn = ws.has_table([kfs[j] for j in nb])
    Tk = np.stack([k["Tcw"] for k in kfs[:n_kf]]); Tn = np.stack([kfs[j]["Tcw"] for j in nb])
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        ws.b.create_new_map_points(np.arange(n_kf), Tk, off, nb, Tn, tc.CAM, d_kf_has_mp=hk.data_ptr(), d_neigh_has_mp=hn.data_ptr(), stream=stream)
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    rec = dict(tool="bench_triangulate", keyframes=n_kf, neighbours=nn, features=int(np.mean([len(k["kp"]) for k in kfs])), timed_calls=a.calls,
               call_ms=round(e0.elapsed_time(e1) / a.calls, 4))
    got = [ws.b.download_new_map_points(k) for k in range(n_kf)]
    rec["new_points"] = int(sum(len(x) for x in got))
    if not a.call_only:
        orc = g.load_oracle()
        tc.attach_bow(kfs, orc.Vocabulary.from_nodes(voc), LEVELSUP)
        tc.oracle()
        t = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            ref = list(pool.map(lambda k: tc.create(kfs[k], kfs[k + 1:k + 1 + nn], lv=ws.lv)["new"], range(n_kf)))
        rec["oracle_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        rec["oracle_threads"] = 16
        rec["identical_to_oracle"] = bool(all(x.tobytes() == y.tobytes() for x, y in zip(got, ref)))
    ws.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
