"""Randomised parity sweep of sd_batch_search_by_bow_kf / sd_batch_search_by_projection_sim3 / sd_batch_fuse_sim3 against the sequential
CPU oracle (developer tool): random scenes of random target count, point count, feature count, pixel noise, level count, radius, scale,
feature states and incoming matches; every output byte for byte.  Integer outputs leave no margin: no case is skipped, a case the
library refuses (the list bound of the projection) counts as a mismatch."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
import triangulate_cases as tc
import fuse_cases as fc
import loop_cases as lc


def run(n_cases, seed0):
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    orc = g.load_oracle()
    rng = np.random.default_rng(seed0)
    voc = tc.vocabulary(synth, 5)
    O = orc.Vocabulary.from_nodes(voc)
    stats = dict(jobs=0, entries=0, fused=0, projected=0, pairs=0, bow_matches=0, skipped=0)
    for nlevels in (8, 12):
        ws = lc.Workspace(fe, 8, voc, dict(tc.GEOM, nlevels=nlevels))
        try:
            for k in range(n_cases):
                nt = int(rng.integers(1, 9)); npts = int(rng.integers(1, 400)); nf = int(rng.integers(1, min(ws.cap, 400)))
                sc = fc.random_scene(1000 * seed0 + k, nt, npts, n_features=nf, mono_share=float(rng.choice([0.0, 0.4, 1.0])),
                                     noise=float(rng.choice([0.0, 0.6, 2.0, 5.0])), lv=ws.lv, shared_list=bool(rng.integers(0, 2)),
                                     state_share=float(rng.choice([0.0, 0.3, 1.0])))
                sc = lc.with_scale(sc, float(rng.choice([1.0, 0.5, 2.0, 1.37, rng.uniform(0.3, 3.0)])))
                rows = lc.matched_from_state(sc)
                for q, (kf, entries, state) in enumerate(sc["jobs"]):       # a few features hold candidates of the job's own list
                    occ = np.nonzero(rows[q] == -2)[0]; cands = entries[entries >= 0]
                    if len(occ) and len(cands):
                        pick = rng.permutation(occ)[:min(4, len(cands))]
                        rows[q][pick] = rng.choice(cands, len(pick), replace=False)
                sc["matched"] = rows
                sc["th"] = float(rng.choice([2.0, 3.0, 4.0, 10.0])); sc["th_proj"] = int(rng.choice([3, 10, 15]))
                try:
                    want, _ = lc.cpu_fuse(sc, lv=ws.lv)
                    fc.assert_same(sc, lc.device_fuse(ws, sc), want)
                    pw, _ = lc.cpu_project(sc, lv=ws.lv)
                    lc.assert_same_project(sc, lc.device_project(ws, sc, upload=False), pw)
                    c = lc.random_bow_case(voc, O, 100 * seed0 + k, n_points=int(rng.integers(20, 350)))
                    (m, nm), = lc.device_bow(ws, [c])
                    wm, wn, _ = lc.cpu_bow(c)
                    assert nm == wn and m.tobytes() == wm.tobytes(), "SearchByBoW: %d vs %d matches" % (nm, wn)
                except (AssertionError, fe.SdError) as e:
                    print("MISMATCH levels %d case %d (%s, th %g / %d): %s" % (nlevels, k, sc["name"], sc["th"], sc["th_proj"], e))
                    return 1
                stats["jobs"] += len(want); stats["entries"] += sum(len(w[0]) for w in want); stats["fused"] += sum(w[2] for w in want)
                stats["projected"] += sum(w[2] for w in pw); stats["pairs"] += 1; stats["bow_matches"] += wn
        finally:
            ws.close()
    print("fuzz_loop: %d cases identical, none skipped" % (2 * n_cases), stats)
    return 0


if __name__ == "__main__":
    sys.exit(run(int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 3))
