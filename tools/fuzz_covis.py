"""Random maps through the device covisibility graph (sd_covis_*) and the sequential CPU oracle (tests/cpp/covis_oracle.cpp): scripts of
mutations (matches, bad flags, parents, erases) and the three queries, compared item by item (nothing here has a tolerance).  Counts
mismatches and skips -- no skip is expected -- and writes profiles/covis_fuzz.json; prints the record as ONE JSON line and exits non-zero
on a mismatch.  Sizes are drawn per seed: keyframes, features per keyframe, points (sparse to dense sharing) and rounds."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import covis_cases as cc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first-seed", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_fuzz.json"))
    a = ap.parse_args()
    fe = g.load_package().frontend
    if fe.device_count() < 1:
        raise SystemExit("fuzz_covis needs a HIP device")
    rec = dict(tool="fuzz_covis", seeds=a.seeds, first_seed=a.first_seed, scripts=0, updates=0, cull_candidates=0, flagged=0, local_maps=0, mismatches=0,
               skipped=0, failures=[])
    for seed in range(a.first_seed, a.first_seed + a.seeds):
        rng = np.random.default_rng(seed)
        n_kf = int(rng.choice([12, 40, 150]))
        n_feat = int(rng.choice([20, 60, 200]))
        n_points = int(n_kf * n_feat * rng.choice([0.05, 0.15, 0.4])) + 8
        ops = cc.random_script(seed, n_kf=n_kf, n_feat=n_feat, n_points=n_points, rounds=int(rng.choice([2, 4, 6])))
        want, br = cc.run_oracle(ops)
        try:
            got = cc.run_device(fe, ops, device=bool(seed & 1))
        except fe.SdError as e:
            rec["skipped"] += 1
            rec["failures"].append(dict(seed=seed, error=str(e)))
            continue
        rec["scripts"] += 1
        rec["updates"] += sum(len(op[1]) for op in ops if op[0] == "update")
        for r in want[:-1]:
            if r[0] == "cull":
                rec["cull_candidates"] += len(r[1]); rec["flagged"] += sum(x[0] for x in r[1])
            elif isinstance(r, list):
                rec["local_maps"] += len(r)
        if cc.differs(got, want):
            rec["mismatches"] += 1
            rec["failures"].append(dict(seed=seed, error="differs from the oracle"))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    sys.exit(1 if rec["mismatches"] or rec["skipped"] else 0)


if __name__ == "__main__":
    main()
