"""Random PnPsolver problems through the device path and the CPU oracle; the summary goes to profiles/pnp_fuzz.json and is printed as ONE
JSON line.  usage: fuzz_pnp.py [problems] [seed] [--cpu]
Two comparisons per draw (DESIGN Q46):
  * against the oracle in the KERNEL's summation order: the whole record and the mask, byte for byte.  Nothing is skipped.
  * against the oracle in the reference's SEQUENTIAL order: kind, iteration, n_inliers and the mask.  A draw is skipped only when the
    oracle's own two orders disagree on one of them; at most 5 % of a sweep may be skipped.
--cpu runs the oracle side alone (the skip share is a property of the oracle and the draws, so it is known before any GPU run).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import pnp_cases as pc  # noqa: E402


def main():
    argv = [x for x in sys.argv[1:] if x != "--cpu"]
    cpu_only = "--cpu" in sys.argv
    n_prob = int(argv[0]) if len(argv) > 0 else 400
    seed = int(argv[1]) if len(argv) > 1 else 1
    rng = np.random.default_rng([2026, seed])
    probs = [pc.random_problem(rng) for _ in range(n_prob)]
    rec = dict(tool="fuzz_pnp", seed=seed, device=not cpu_only, problems=n_prob, correspondences=int(sum(len(p["corr"]) for p in probs)))
    fe = None
    if not cpu_only:
        fe = g.load_package().frontend
        if fe.device_count() < 1:
            raise SystemExit("fuzz_pnp needs a HIP device (or --cpu)")
    groups = {}
    for pr in probs:
        groups.setdefault(pc.group_key(pr), []).append(pr)
    kinds = {0: 0, 1: 0, 2: 0}
    mism_tree, mism_seq, skipped, refines = [], [], 0, 0
    for key, prs in groups.items():
        kw = dict(zip(("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2"), key))
        seq = [pc.iterate(p, order=0) for p in prs]
        tree = [pc.iterate(p, order=1) for p in prs]
        dec = lambda r, i: (int(r["kind"]), int(r["iteration"]), int(r["n_inliers"]), i.tobytes())
        agree = [dec(s[0], s[1]) == dec(t[0], t[1]) for s, t in zip(seq, tree)]
        skipped += len(prs) - sum(agree)
        for s in seq:
            kinds[int(s[0]["kind"])] += 1; refines += s[2]["refine_calls"]
        if cpu_only:
            continue
        off, corr, tab = pc.pack(prs)
        res, inl = fe.pnp_ransac(off, corr, tab, **kw)
        for k in range(len(prs)):
            gi = inl[off[k]:off[k + 1]]
            if not (pc.same_result(res[k], tree[k][0]) and gi.tobytes() == tree[k][1].tobytes()):
                mism_tree.append(dict(group=list(key), index=k, n=int(off[k + 1] - off[k])))
            if agree[k] and dec(res[k], gi) != dec(seq[k][0], seq[k][1]):
                mism_seq.append(dict(group=list(key), index=k, n=int(off[k + 1] - off[k])))
    rec.update(kinds={str(k): v for k, v in kinds.items()}, sequential_refine_calls=int(refines), compared=0 if cpu_only else n_prob,
               skipped_against_sequential=skipped, skipped_share=round(skipped / max(n_prob, 1), 4), mismatches_kernel_order=mism_tree[:10],
               n_mismatches_kernel_order=len(mism_tree), mismatches_sequential=mism_seq[:10], n_mismatches_sequential=len(mism_seq))
    if not cpu_only:
        with open(os.path.join(ROOT, "profiles", "pnp_fuzz.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))
    if mism_tree or mism_seq or rec["skipped_share"] > 0.05:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
