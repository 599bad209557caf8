"""Randomised parity sweep of sd_batch_search_by_projection_reloc and sd_batch_relocalize_refine against the sequential CPU oracle
(developer tool), written to profiles/reloc_fuzz.json.
Matcher draws: random scenes (feature counts, poses, held features, found flags, bad points, th / ORBdist), every output byte for byte;
none is skipped, and a draw the library refuses (the list bound) counts as a mismatch.
Cascade draws: every draw is checked stage by stage (each search byte for byte from the device's own stage pose, each optimisation
against the pose oracle within pose_close's 1e-5).  The free-running comparison -- stage_reached, matched, n_good, n_additional, the
final assignment and flags against the oracle run on its own poses -- is skipped for a draw whose oracle decisions change under a
perturbation of that size; skips are counted, reported, and may not exceed 5 % of the draws."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402
import triangulate_cases as tc  # noqa: E402
import reloc_cases as rc  # noqa: E402


def run(n_cases, seed0, out):
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    rng = np.random.default_rng(seed0)
    ws = rc.Workspace(fe, 8, tc.vocabulary(synth, 5))
    stats = dict(tool="fuzz_reloc", seed=seed0, matcher_draws=0, matcher_jobs=0, matcher_matches=0, matcher_skipped=0, cascade_draws=0, cascade_jobs=0,
                 cascade_skipped=0, cascade_matched=0, stages_reached={})
    try:
        for k in range(n_cases):
            sc = rc.random_scene(1000 * seed0 + k, n_kf=int(rng.integers(1, 400)), n_frame=int(rng.integers(1, 300)), n_jobs=int(rng.integers(1, 5)))
            for j in sc["jobs"]:
                j["th"] = float(rng.choice([3.0, 10.0, 15.0, 1.5])); j["orb"] = int(rng.choice([64, 100, 255, 30]))
            try:
                want, _ = rc.cpu_search(sc, lv=ws.lv)
                rc.assert_same(sc, rc.device_search(ws, sc), want)
            except (AssertionError, fe.SdError) as e:
                print("MISMATCH matcher draw %d (%s): %s" % (k, sc["name"], e))
                return 1
            stats["matcher_draws"] += 1; stats["matcher_jobs"] += len(want); stats["matcher_matches"] += int(sum(w[4] for w in want))
            cs = rc.random_cascade_scene(1000 * seed0 + k, n_jobs=4)
            try:
                got = rc.device_refine(ws, cs)
                rc.check_stages(ws, cs, cs["jobs"], got, quiet=True)
                free = rc.cpu_refine(cs, lv=ws.lv)
                pert = np.array([rc.pose_perturbation(rng, j["Tcw"]) for j in cs["jobs"]])
                shaken = rc.cpu_refine(cs, perturb=pert, lv=ws.lv)
                for q, (a, b, c) in enumerate(zip(got, free, shaken)):
                    stats["cascade_jobs"] += 1
                    st = str(int(b[0]["stage_reached"])); stats["stages_reached"][st] = stats["stages_reached"].get(st, 0) + 1
                    stats["cascade_matched"] += int(b[0]["matched"])
                    if rc.decisions(b) != rc.decisions(c):
                        stats["cascade_skipped"] += 1
                        continue
                    n2 = len(b[1])
                    assert rc.decisions((a[0], a[1][:n2], a[2][:n2])) == rc.decisions(b), "cascade job %d: free-running decisions differ" % q
            except (AssertionError, fe.SdError) as e:
                print("MISMATCH cascade draw %d (%s): %s" % (k, cs["name"], e))
                return 1
            stats["cascade_draws"] += 1
    finally:
        ws.close()
    stats["cascade_skip_share"] = round(stats["cascade_skipped"] / max(stats["cascade_jobs"], 1), 4)
    if stats["cascade_skipped"] * 20 > stats["cascade_jobs"]:
        print("fuzz_reloc: too many cascade draws hang on the pose", stats)
        return 1
    with open(out, "w") as f:
        json.dump(stats, f, indent=1)
        f.write("\n")
    print("fuzz_reloc: every draw identical", json.dumps(stats))
    return 0


if __name__ == "__main__":
    sys.exit(run(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 3,
                 sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "reloc_fuzz.json")))
