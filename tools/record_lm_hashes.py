"""Record SHA-256 of what the three Levenberg-Marquardt kernels (k_pose_optimize, k_local_ba, k_sim3_optimize) and the chains built on
them (the ComputeSim3 refine chain, the relocalisation cascade) answer on the project's crafted cases: tests/golden/lm_parent_hashes.json.

    python tools/record_lm_hashes.py <commit> [out.json]

Run it ONCE from a checkout of the commit whose results are the yardstick (the parent of a change to the solvers' shared arithmetic,
csrc/sd_g2o_math.h) and name that commit; tests/test_gpu_lm_parent.py compares against the file, which is never regenerated from the code
under test.  The groups are defined here and imported by the test; every group is one function (fe, synth) -> {case: digest}, a digest
being the SHA-256 over the bytes of every output array of the case in the order listed:
  pose_crafted    every case of tests/pose_crafted.py in one sd_pose_optimize_host launch, each with its own camera (all four quaternion
                  branches, the not-positive solve, the nE < 3 and nE < 10 exits, rejected last trials): Tcw, outlier flags, nGood
  pose_cases      the seeded problems of tests/pose_cases.py over test_gpu_pose.py's grid (size x mono / stereo / mixed x outlier ratio x
                  perturbation) in one sd_pose_optimize_host launch, a digest per size: Tcw, outlier flags, nGood of its 27 problems
  pose_workspace  sd_batch_pose_optimize (the launcher with the `map` indirection) on pose_crafted's uploaded frames and match rows, a
                  digest per pair: Tcw, mvbOutlier per keypoint, nInitialCorrespondences, the return value
  ba              every case of tests/ba_cases.py in one sd_local_ba_host launch: poses, points, normals, distances, level1, erase, stats
  sim3_opt        every crafted case of tests/sim3_opt_cases.py in one sd_sim3_optimize_host launch: the result record, the state bytes
  sim3_refine     sd_batch_compute_sim3_refine on test_gpu_sim3_refine.py's first scene, a digest per job: result, final12, then the
                  stages (merged12, the built correspondences, the optimiser's state bytes)
  reloc           sd_batch_relocalize_refine (the third launcher of k_pose_optimize) on reloc_cases.cascade_scene(), a digest per job:
                  result, the final assignment, the outlier flags."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

POSE_SIZES = (0, 1, 2, 3, 5, 9, 10, 11, 37, 64, 257, 1000, 2000, 8000)      # test_gpu_pose.py's grid
REFINE_SCENE = dict(seed=3, n_points=300, n_jobs=3, not_found=(1,))
SLOTS = 24                                                                   # two per cascade case; the other scenes need fewer


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pose_crafted(fe, synth):
    import pose_crafted as pcr
    names = pcr.names()
    cs = [pcr.cases()[n] for n in names]
    off = np.zeros(len(cs) + 1, np.int32)
    off[1:] = np.cumsum([len(c["edges"]) for c in cs])
    T, out, good = fe.pose_optimize(off, np.concatenate([c["edges"] for c in cs]), [c["cam"] for c in cs], np.stack([c["T0"] for c in cs]))
    return {n: digest([T[k], out[off[k]:off[k + 1]], good[k:k + 1]]) for k, n in enumerate(names)}


def pose_cases(fe, synth):
    import pose_cases as pc
    rng = np.random.default_rng(2024)
    probs = []
    for n in POSE_SIZES:
        for kind in ("mono", "stereo", "mixed"):
            for ratio in (0.0, 0.3, 0.6):
                for pert in ((0, 0), (2, 0.05), (10, 0.5)):
                    e, T, _ = pc.make_problem(rng, n, kind, ratio, noise=1.0)
                    probs.append((e, pc.perturb(T, rng, *pert).astype(np.float32)))
    off = np.zeros(len(probs) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e, _ in probs])
    T, out, good = fe.pose_optimize(off, np.concatenate([e for e, _ in probs]), pc.CAM, np.stack([T for _, T in probs]))
    per = len(probs) // len(POSE_SIZES)
    return {"n=%d" % n: digest([T[k * per:(k + 1) * per], out[off[k * per]:off[(k + 1) * per]], good[k * per:(k + 1) * per]])
            for k, n in enumerate(POSE_SIZES)}


def pose_workspace(fe, synth, ws):
    import torch
    import pose_crafted as pcr
    import triangulate_cases as tc
    frames = [pcr.edge_frames(N, 900 + k, ws.ex.mvInvLevelSigma2) for k, N in enumerate(pcr.FRAME_SIZES)]
    P = len(frames)
    kfs = [None] * (2 * P)
    for q, f in enumerate(frames):
        kfs[2 * q], kfs[2 * q + 1] = f["last"], f["cur"]
    ws.upload_grid(kfs, tc.CAM)
    for q, f in enumerate(frames):
        ws.b.set_mappoints(2 * q, f["xw"], f["flags"])
    I = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    ws.b.search_by_projection([2 * q + 1 for q in range(P)], [2 * q for q in range(P)], I, I, tc.CAM, 15.0)     # the pairs exist
    ws.b.sync()
    d_match, _, _, _, cap = ws.b.matches_device()                  # the crafted match rows over the matcher's
    full = np.full((P, cap), -1, np.int32)
    for q, f in enumerate(frames):
        full[q, :len(f["match"])] = f["match"]
    fe.as_torch_u8(d_match, P * cap * 4).view(torch.int32).view(P, cap).copy_(torch.from_numpy(full).cuda())
    torch.cuda.synchronize()
    ws.b.pose_optimize(list(range(P))[::-1], Tcw=np.stack([f["T0"] for f in frames])[::-1])       # workgroup p works on pair map[p] != p
    out = {}
    for q, f in enumerate(frames):
        Tg, og, ni, ng = ws.b.download_pose(q)
        out["N=%d" % len(f["match"])] = digest([Tg, og, np.array([ni, ng], np.int32)])
    return out


def ba(fe, synth):
    import ba_cases as bc
    names = list(bc.CASES)
    got = fe.local_bundle_adjustment([bc.problem_of(bc.scene(n)) for n in names])
    return {n: digest([g[f] for f in ("Tcw", "xw", "normal", "dist", "level1", "erase", "stats")]) for n, g in zip(names, got)}


def sim3_opt(fe, synth):
    import sim3_opt_cases as sc
    cases = sc.crafted_cases()
    off, corr, probs = sc.pack(cases)
    res, st = fe.sim3_optimize(off, corr, probs)
    return {c["name"]: digest([res[k:k + 1], st[off[k]:off[k + 1]]]) for k, c in enumerate(cases)}


def sim3_refine(fe, synth, ws):
    import sim3_refine_cases as rc
    got = rc.device_refine(ws, rc.refine_scene(**REFINE_SCENE))
    return {"job %d" % q: digest([g["result"], g["final12"], g["merged12"], g["corr"], g["state"]]) for q, g in enumerate(got)}


def reloc(fe, synth, ws):
    import reloc_cases as rl
    sc = rl.cascade_scene()
    got = rl.device_refine(ws, sc)
    return {n: digest([g[0], g[1], g[2]]) for n, g in zip(sc["names"], got)}


PLAIN = (pose_crafted, pose_cases, ba, sim3_opt)                   # (fe, synth)
ON_WORKSPACE = (pose_workspace, sim3_refine, reloc)                # (fe, synth, ws): uploaded frames in a Batch
GROUPS = tuple(g.__name__ for g in PLAIN + ON_WORKSPACE)


def workspace(fe, synth):
    import fuse_cases as fc
    import triangulate_cases as tc
    return fc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    fe, synth = pkg.frontend, pkg.synth
    commit = sys.argv[1]
    if os.path.exists(os.path.join(ROOT, ".git")):                 # a checkout: it has to be the commit it claims, with its sources unchanged
        import subprocess
        git = lambda *a: subprocess.check_output(("git", "-C", ROOT) + a, text=True).strip()
        assert git("rev-parse", "HEAD") == commit, "this checkout is %s, not %s" % (git("rev-parse", "HEAD"), commit)
        assert not git("status", "--porcelain", "--", "slam-dynamic_amd", "include"), "the library's sources differ from " + commit
    else:
        print("no .git here: the commit named is taken on trust (an exported tree)")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "lm_parent_hashes.json")
    rec = {"commit": commit, "cases": {}}
    for g in PLAIN:
        rec["cases"][g.__name__] = g(fe, synth)
    ws = workspace(fe, synth)
    try:
        for g in ON_WORKSPACE:
            rec["cases"][g.__name__] = g(fe, synth, ws)
    finally:
        ws.close()
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%s: %s" % (out, ", ".join("%s: %d" % (k, len(v)) for k, v in rec["cases"].items())))


if __name__ == "__main__":
    main()
