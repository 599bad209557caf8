"""Randomised parity sweep of the TrackHomo model fit against the CPU oracle (developer tool): a draw picks the pair count N
log-uniform in [0, kp_capacity], a scene kind (planar, general, unrelated points), an outlier share in [0, 0.7], a noise in
[0, 2] px and, with probability 0.1, one of the degeneracies of tests/motion_cases.py instead; the sets run on the device in
batches, through the point-set path of the tests (motion_cases.run_sets)."""
import collections
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
import motion_cases as mc


def draw(rng, cap):
    N = min(cap, int(np.exp(rng.uniform(0, np.log(cap + 1.0)))) - 1)
    kind = ("planar", "general", "noise_only")[int(rng.integers(0, 3))]
    frac, noise = float(rng.uniform(0, 0.7)), float(rng.uniform(0, 2.0))
    if rng.random() < 0.1:
        kind = mc.DEGENERATE_KINDS[int(rng.integers(0, len(mc.DEGENERATE_KINDS)))]
        return "%s N=%d" % (kind, N), mc.degenerate(kind, N)
    pts = mc.noise_only(rng, N) if kind == "noise_only" else getattr(mc, kind)(rng, N, frac, noise)
    return "%s N=%d outliers %.2f noise %.2f" % (kind, N, frac, noise), pts


def run(n_draws, seed, n_features=0, n_sets=8):
    """-> number of draws whose device result differs from the oracle.  n_features: the extractor's (0 = the settings file's)."""
    pkg = g.load_package(); orc = g.load_oracle()
    fe, synth = pkg.frontend, pkg.synth
    cfg = dict(synth.KITTI03_RGBD)
    if n_features:
        cfg["n_features"] = n_features
    rng = np.random.default_rng(seed)
    ws = mc.Workspace(fe, synth, cfg, n_sets)
    stats = collections.Counter()
    failures = 0
    try:
        draws = [draw(rng, ws.cap) for _ in range(n_draws)]
        got = mc.run_all(ws, [pts for _, pts in draws])
        for (name, (p1, p2)), gm in zip(draws, got):
            o = orc.estimate_motion_ex(p1, p2)
            bad, dh, df, same = mc.compare(gm, o)
            stats["flag %d" % o["flag"]] += 1; stats["bit-identical"] += int(same); stats["over 2048 pairs"] += int(len(p1) > 2048)
            stats["H stopped at the checkpoint"] += int(o["stop_h"]); stats["F stopped at the checkpoint"] += int(o["stop_f"])
            stats["with degenerate hypotheses"] += int(o["deg_h"] + o["deg_f"] > 0)
            if bad:
                failures += 1
                print("MISMATCH %s (seed %d): %s" % (name, seed, "; ".join(bad)))
    finally:
        ws.close()
    print("fuzz_motion: %d draws, %d differ (capacity %d)" % (n_draws, failures, ws.cap), dict(stats))
    return failures


if __name__ == "__main__":
    sys.exit(min(1, run(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 3,
                        int(sys.argv[3]) if len(sys.argv) > 3 else 0)))
