"""Randomised parity sweep of sd_local_ba_host against the sequential CPU oracle (developer tool): random scenes of ba_cases.random_scene
(keyframe, point and edge counts, stereo share, noise, start error, planted outliers) through frontend.local_bundle_adjustment, all of a
sweep in one launch, compared as tests/test_gpu_ba.py compares the crafted cases (decisions and counts exactly, values within
max(10 x the problem's own spread, 4 f32 ulps)).  A problem with a decision inside the relative margin of 1e-6, or whose oracle variants
disagree, is skipped and counted; more than 2 % skipped means the generator is wrong.  Prints one JSON line and, with a third argument,
writes it to that file (profiles/ba_fuzz.json holds the recorded run)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import ba_cases as bc  # noqa: E402


def run(n_cases, seed0, out=None):
    fe = g.load_package().frontend
    scenes = [bc.random_scene(100000 * seed0 + k) for k in range(n_cases)]
    probs = [bc.problem_of(s) for s in scenes]
    want = [bc.run_oracle(p) for p in probs]
    got = fe.local_bundle_adjustment(probs)
    skipped = compared = 0
    stats = dict(edges=0, trials=0, rejected=0, erased=0)
    for k in range(n_cases):
        sp = bc.spread_of(probs[k], want[k]) if min(want[k]["margins"].values()) >= bc.MARGIN else None
        if sp is None:
            skipped += 1
            continue
        bad = bc.mismatch(got[k], want[k], sp)
        if bad:
            print("MISMATCH seed %d: %s" % (100000 * seed0 + k, bad))
            return 1
        compared += 1
        stats["edges"] += len(probs[k]["edges"]); stats["trials"] += int(want[k]["stats"]["trials"].sum())
        stats["rejected"] += int(want[k]["stats"]["rejected"].sum()); stats["erased"] += int(want[k]["stats"]["n_erased"])
    rec = dict(tool="fuzz_ba", problems=n_cases, first_seed=100000 * seed0, compared=compared, skipped=skipped,
               skipped_share=round(skipped / n_cases, 4), mismatches=0, **stats)
    print(json.dumps(rec))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    if skipped > 0.02 * n_cases:
        print("fuzz_ba: %d of %d problems skipped: the generator is wrong" % (skipped, n_cases))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(run(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 3, sys.argv[3] if len(sys.argv) > 3 else None))
