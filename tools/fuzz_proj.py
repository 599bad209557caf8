"""Randomised parity sweep of the two projection matchers against the CPU oracle (developer tool): the seeded random scenes of
tests/proj_cases.py -- poses, depths, octaves, flags, occupied key points, mono and stereo key points, prototype descriptors with flipped
bits, th, nnratio, bMono -- through sd_batch_search_by_projection and sd_batch_search_local_map, compared byte for byte.
usage: python tools/fuzz_proj.py [n_scenes [first_seed]]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g


def run(n_scenes, seed0):
    import fuse_cases as fc
    import proj_cases as pc
    import triangulate_cases as tc
    pkg = g.load_package(); orc = g.load_oracle()
    ws = fc.Workspace(pkg.frontend, 8, tc.vocabulary(pkg.synth, 5))
    points = 0
    try:
        for seed in range(seed0, seed0 + n_scenes):
            sc = pc.random_ff_scene(seed)
            for P, got in zip(sc["pairs"], pc.device_ff(ws, sc)):
                try:
                    pc.same_ff(got, pc.oracle_ff(orc, P, sc["th"], sc["bMono"]), P["name"])
                except AssertionError as e:
                    print("MISMATCH seed %d (th %.0f bMono %d): %s" % (seed, sc["th"], sc["bMono"], e))
                    return 1
                points += len(P["xw"])
            sc = pc.random_lm_scene(seed)
            for F, got in zip(sc["frames"], pc.device_lm(ws, sc)):
                try:
                    pc.same_lm(got, pc.oracle_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"]), F["name"])
                except AssertionError as e:
                    print("MISMATCH seed %d (th %.0f nnratio %.1f limit %.2f): %s" % (seed, sc["th"], sc["nnratio"], sc["cos_limit"], e))
                    return 1
                points += len(F["points"])
    finally:
        ws.close()
    print("fuzz_proj: %d scenes of each matcher identical (%d points)" % (n_scenes, points))
    return 0


if __name__ == "__main__":
    sys.exit(run(int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 100))
