"""Random Sim3Solver problems and SearchBySim3 scenes through the device path and the sequential CPU oracle, byte for byte; the summary
goes to profiles/sim3_fuzz.json and is printed as ONE JSON line.  usage: fuzz_sim3.py [problems] [scenes] [seed] [--cpu]
Nothing is skipped for rounding: device and oracle are specified to the byte (DESIGN Q39), so every problem and scene is compared.  The
one skip there is: a scene one of whose keyframes holds more key points than the workspace (counted, with the reason, and bounded at
2 % of the cases).  --cpu runs the oracle side alone and applies the same skip rule against the least capacity a workspace of that
geometry can have (its feature count), so the skipped share it reports is an upper bound of the device run's.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import triangulate_cases as tc  # noqa: E402
import fuse_cases as fc  # noqa: E402
import sim3_cases as sc  # noqa: E402


def main():
    argv = [x for x in sys.argv[1:] if x != "--cpu"]
    cpu_only = "--cpu" in sys.argv
    n_prob = int(argv[0]) if len(argv) > 0 else 400
    n_scene = int(argv[1]) if len(argv) > 1 else 12
    seed = int(argv[2]) if len(argv) > 2 else 1
    rng = np.random.default_rng([2026, seed])
    probs = [sc.random_problem(rng) for _ in range(n_prob)]
    rec = dict(tool="fuzz_sim3", seed=seed, device=not cpu_only)
    fe = synth = None
    if not cpu_only:
        pkg = g.load_package()
        fe, synth = pkg.frontend, pkg.synth
        if fe.device_count() < 1:
            raise SystemExit("fuzz_sim3 needs a HIP device (or --cpu)")
    # ---- RANSAC: one call per argument group
    groups = {}
    for pr in probs:
        groups.setdefault((pr["probability"], pr["min_inliers"], pr["max_iterations"]), []).append(pr)
    branches = {"none": 0, "found": 0, "exhausted": 0}
    mism, hyp = [], 0
    for (pb, mi, mx), prs in groups.items():
        ref = [sc.find(p) for p in prs]
        for r, _, info in ref:
            branches[sc.BRANCH[int(info[0])]] += 1; hyp += int(info[1])
        if cpu_only:
            continue
        off, corr, tab = sc.pack(prs)
        res, inl = fe.sim3_ransac(off, corr, tab, pb, mi, mx)
        for k, (r, io, _) in enumerate(ref):
            if not (sc.same_result(res[k], r) and inl[off[k]:off[k + 1]].tobytes() == io.tobytes()):
                mism.append(dict(group=[pb, mi, mx], index=k, n=int(off[k + 1] - off[k])))
    rec["ransac"] = dict(problems=n_prob, correspondences=int(sum(len(p["corr"]) for p in probs)), sequential_hypotheses=hyp, branches=branches,
                         compared=0 if cpu_only else n_prob, skipped=0, mismatches=mism[:10], n_mismatches=len(mism))
    # ---- SearchBySim3
    ws = None if cpu_only else fc.Workspace(fe, 8, tc.vocabulary(synth, 5))
    cap = ws.cap if ws else tc.GEOM["nfeatures"]          # without a device: the extractor's feature count, which no workspace's capacity is below
    skipped, why, found, smis, pairs = 0, [], 0, [], 0
    totals = {k: 0 for k in sc.S3_COUNTERS}
    for k in range(n_scene):
        scene = sc.random_search_scene(int(rng.integers(1 << 30)), int(rng.integers(50, 420)), int(rng.integers(1, 5)),
                                       noise=float(rng.uniform(0.2, 2.0)), share_matched=float(rng.uniform(0, 0.6)))
        if max(len(f["kp"]) for f in scene["kfs"]) > cap:
            skipped += 1; why.append("scene %d: a keyframe holds more key points than the workspace" % k)
            continue
        want, cnt = sc.cpu_search(scene)
        pairs += len(want); found += sum(w[3] for w in want)
        for name in totals:
            totals[name] = max(totals[name], cnt[name]) if name.endswith("_max") else totals[name] + cnt[name]
        if cpu_only:
            continue
        got = sc.device_search(ws, scene)
        try:
            sc.assert_same_search(scene, got, want)
        except AssertionError as e:
            smis.append(str(e)[:200])
    if ws:
        ws.close()
    rec["search"] = dict(scenes=n_scene, pairs=pairs, found=int(found), counters=totals, compared=0 if cpu_only else n_scene - skipped,
                         skipped=skipped, skipped_why=why, mismatches=smis[:10], n_mismatches=len(smis))
    rec["skipped_share"] = round(skipped / max(n_prob + n_scene, 1), 4)
    if not cpu_only:
        with open(os.path.join(ROOT, "profiles", "sim3_fuzz.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))
    if mism or smis or rec["skipped_share"] > 0.02:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
