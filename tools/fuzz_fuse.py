"""Randomised parity sweep of sd_batch_fuse / sd_distinctive_descriptors_device against the sequential CPU oracle (developer tool):
synthetic scenes of random target count, point count, feature count, mono share, pixel noise, level count, search radius and feature
states; (bestIdx, bestDist) of every entry, every sd_fuse_hit record and every return value byte for byte."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
import triangulate_cases as tc
import fuse_cases as fc


def run(n_cases, seed0):
    import torch
    pkg = g.load_package()
    fe, synth = pkg.frontend, pkg.synth
    rng = np.random.default_rng(seed0)
    voc = tc.vocabulary(synth, 5)
    stats = dict(jobs=0, entries=0, fused=0, points=0)
    for nlevels in (8, 12):
        ws = fc.Workspace(fe, 12, voc, dict(tc.GEOM, nlevels=nlevels))
        try:
            for k in range(n_cases):
                nt = int(rng.integers(1, 13)); npts = int(rng.integers(1, 500)); nf = int(rng.integers(1, min(ws.cap, 500)))
                sc = fc.random_scene(1000 * seed0 + k, nt, npts, n_features=nf, mono_share=float(rng.choice([0.0, 0.4, 1.0])),
                                     noise=float(rng.choice([0.0, 0.6, 2.0])), lv=ws.lv, shared_list=bool(rng.integers(0, 2)),
                                     state_share=float(rng.choice([0.0, 0.3, 1.0])))
                sc["th"] = float(rng.choice([2.0, 3.0, 4.0, 10.0]))
                want, _ = fc.cpu_run(sc, lv=ws.lv)
                got = fc.device_run(ws, sc)
                try:
                    fc.assert_same(sc, got, want)
                except AssertionError as e:
                    print("MISMATCH levels %d case %d (%s, th %g): %s" % (nlevels, k, sc["name"], sc["th"], e))
                    return 1
                stats["jobs"] += len(want); stats["entries"] += sum(len(w[0]) for w in want); stats["fused"] += sum(w[2] for w in want)
                # ComputeDistinctiveDescriptors of random observation sets
                lists = [rng.integers(0, 256, (int(rng.integers(0, 90)), 32), dtype=np.uint8) for _ in range(50)]
                off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
                d = torch.from_numpy(np.concatenate(lists + [np.zeros((1, 32), np.uint8)]).reshape(-1)).cuda()
                best = torch.zeros(len(lists), dtype=torch.int32).cuda()
                keep = fe.distinctive_descriptors(off, d.data_ptr(), best.data_ptr())
                torch.cuda.synchronize()
                ref = [fc.distinctive(x)[0] for x in lists]
                if best.cpu().tolist() != ref:
                    print("MISMATCH levels %d case %d: distinctive descriptors" % (nlevels, k))
                    return 1
                stats["points"] += len(lists)
                del keep
        finally:
            ws.close()
    print("fuzz_fuse: %d cases identical" % (2 * n_cases), stats)
    return 0


if __name__ == "__main__":
    sys.exit(run(int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 3))
