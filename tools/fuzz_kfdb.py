"""Random databases through the device KeyFrameDatabase (sd_kfdb_*) and the sequential CPU oracle (tests/cpp/kfdb_oracle.cpp), both query
forms and the score helper, compared byte for byte (nothing here has a tolerance).  Counts mismatches and skips -- no skip is expected --
and writes profiles/kfdb_fuzz.json; prints the record as ONE JSON line and exits non-zero on a mismatch.
Every script interleaves add / erase / re-add with neighbour updates and calls of several queries; sizes are drawn per seed: the
vocabulary (dense to sparse sharing), the words per entry (1 .. a few hundred) and the queries per call."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import kfdb_cases as kc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first-seed", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_fuzz.json"))
    a = ap.parse_args()
    fe = g.load_package().frontend
    if fe.device_count() < 1:
        raise SystemExit("fuzz_kfdb needs a HIP device")
    rec = dict(tool="fuzz_kfdb", seeds=a.seeds, first_seed=a.first_seed, scripts=0, queries=0, scored=0, candidates=0, mismatches=0, skipped=0, failures=[])
    for seed in range(a.first_seed, a.first_seed + a.seeds):
        rng = np.random.default_rng(seed)
        max_kf = int(rng.choice([64, 200, 500]))
        n_entries = int(max_kf * rng.uniform(0.3, 0.8))
        vocab = int(rng.choice([80, 600, 5000]))
        hi = int(rng.choice([8, 60, 300]))
        qpc = int(rng.choice([1, 3, 8]))
        ops = kc.random_script(seed, n_entries=n_entries, max_kf=max_kf, vocab=vocab, words=(1, min(hi, vocab)), n_calls=4, queries_per_call=qpc)
        want, br = kc.run_oracle(ops, max_kf)
        try:
            got = kc.run_device(fe, ops, max_kf, max_queries=qpc, device=bool(seed & 1))
        except fe.SdError as e:
            rec["skipped"] += 1
            rec["failures"].append(dict(seed=seed, error=str(e)))
            continue
        rec["scripts"] += 1
        for call in want[:-1]:
            for r in call:
                if isinstance(r, dict):
                    rec["queries"] += 1; rec["scored"] += int(r["info"]["nscores"]); rec["candidates"] += int(r["info"]["n_candidates"])
        if kc.differs(got, want):
            rec["mismatches"] += 1
            rec["failures"].append(dict(seed=seed, error="differs from the oracle"))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    sys.exit(1 if rec["mismatches"] or rec["skipped"] else 0)


if __name__ == "__main__":
    main()
