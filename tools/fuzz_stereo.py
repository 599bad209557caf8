"""Randomised parity sweep of the device stereo matcher against the CPU oracle (developer tool): a draw picks a geometry of
tests/stereo_cases.py, key-point counts log-uniform in [0, kp_capacity] on either side, a scene disparity, a noise amplitude
and a descriptor bit-flip rate, optionally squeezes the key points into a few rows (several staging passes), puts them on integer
positions, lets partners lie where their SAD window is refused or moves them off their place by whole pixels of their level; the cases run on the device in batches through the crafted-key-point path of the tests (stereo_cases.run_cases).
Prints the histogram of outcomes that the oracle reports and stops at the first byte that differs.

    python tools/fuzz_stereo.py [draws per geometry = 48] [seed = 5]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g_
import stereo_cases as sc


def draw(rng, g, cap, k):
    d = int(rng.choice([0, 1, 2, 5, 9, 17, 40, 120, int(g.maxD) - 2, int(g.maxD) + 2]))
    amp = int(rng.choice([0, 1, 3, 8, 25]))
    flip_hi = int(rng.choice([0, 40, 74, 75, 110, 140]))
    n = min(cap, int(np.exp(rng.uniform(0, np.log(cap + 1.0)))) - 1)
    extra_l, extra_r = [min(cap - n, int(np.exp(rng.uniform(0, np.log(cap + 1.0)))) - 1) * int(rng.random() < 0.4) for _ in range(2)]
    left, right = sc.images(g, "copy", d)
    if amp:
        right = np.clip(right.astype(np.int64) + rng.integers(-amp, amp + 1, right.shape), 0, 255).astype(np.uint8)
    squeeze = rng.random() < 0.3
    y_lo = int(rng.integers(0, g.H - 40)) if squeeze else 0
    kL, dL, kR, dR = sc.pairs(g, rng, n, d, flips=(0, flip_hi), jitter=bool(rng.random() < 0.7), y_lo=y_lo,
                              y_hi=y_lo + int(rng.integers(2, 40)) if squeeze else None, windowed=bool(rng.random() < 0.6))
    if rng.random() < 0.4:                                          # partners off their place by up to 6 pixels of their level: edge shifts
        kR["x"] = np.clip(kR["x"] + rng.integers(-6, 7, len(kR)) * g.scale[kR["octave"]], 0, np.float32(g.W - 1))
    for side, extra in ((0, extra_l), (1, extra_r)):
        ke = sc.kps(g, rng.uniform(0, g.W - 0.01, extra), rng.uniform(y_lo, (y_lo + 40 if squeeze else g.H) - 0.01, extra),
                    rng.integers(0, g.n_levels, extra))
        de = sc.rand_desc(rng, extra)
        if side == 0:
            kL, dL = np.concatenate([kL, ke]), np.concatenate([dL, de])
        else:
            kR, dR = np.concatenate([kR, ke]), np.concatenate([dR, de])
    pr = rng.permutation(len(kR))                                   # right indices in no particular order
    name = "fuzz%d-d%d-noise%d-flips%d-n%d+%d+%d%s" % (k, d, amp, flip_hi, n, extra_l, extra_r, "-squeezed" if squeeze else "")
    return sc.check_domain(sc.case(g, name, (left, right), kL, dL, kR[pr], dR[pr]), cap)


def run(n_draws, seed, frames=16):
    """-> number of cases whose device result differs from the oracle."""
    pkg = g_.load_package(); orc = g_.load_oracle()
    fe = pkg.frontend
    hist = np.zeros(10, np.int64)
    total = kps = failures = 0
    for gi, g in enumerate(sc.GEOMS.values()):
        rng = np.random.default_rng([seed, gi])
        ws = sc.Workspace(fe, g, frames)
        try:
            for k0 in range(0, n_draws, frames):
                cases = [draw(rng, g, ws.cap, k) for k in range(k0, min(k0 + frames, n_draws))]
                got = sc.run_cases(ws, cases)
                for c, r in zip(cases, got):
                    eL = orc.Extractor(*g.extractor_args()); eR = orc.Extractor(*g.extractor_args())
                    eL(c["left"]); eR(c["right"])
                    o = orc.stereo_matches_ex(eL, eR, c["kL"], c["dL"], c["kR"], c["dR"], g.bf, g.fx)
                    hist += np.bincount(o["outcome"], minlength=10); total += 1; kps += len(c["kL"])
                    bad = sc.compare(r, o)
                    if bad:
                        failures += 1
                        print("MISMATCH %s (seed %d): %s" % (c["name"], seed, "; ".join(bad)))
                        raise SystemExit(1)
        finally:
            ws.close()
    print("fuzz_stereo: %d cases over %d geometries, %d left key points, %d differ (seed %d);" % (total, len(sc.GEOMS), kps, failures, seed),
          dict(zip(orc.ST_NAMES, hist.tolist())))
    return failures


if __name__ == "__main__":
    sys.exit(min(1, run(int(sys.argv[1]) if len(sys.argv) > 1 else 48, int(sys.argv[2]) if len(sys.argv) > 2 else 5)))
