"""Randomised parity sweep of the extractor against the CPU oracle (developer tool; a few fixed draws are in tests/).
python tools/fuzz_extract.py [cases [seed]] [--crafted]: --crafted draws the crafted kinds of tests/extract_cases.py instead of textures
(lattices with random phase, modulus and amplitude, sparse dots, plateaus of equal values) with nfeatures down to 1."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

def draw(rng):
    w = int(rng.integers(160, 1400)); h = int(rng.integers(120, 520))
    scale = float(rng.choice([1.1, 1.15, 1.2, 1.25, 1.3, 1.4, 1.5, 1.7, 2.0]))
    w = max(w, h + 1)                                                          # landscape (portrait levels are undefined in the reference)
    lmax = 1 + int(np.floor(np.log(min(w, h) / 64.0) / np.log(scale)))         # smallest level keeps at least one 30-px cell row
    levels = int(rng.integers(1, max(2, min(8, lmax) + 1)))
    nf = int(rng.integers(100, 2500)) if levels > 2 else int(rng.integers(100, 1200))
    ini = int(rng.integers(8, 40)); mn = int(rng.integers(2, ini + 1))
    kind = str(rng.choice(["texture", "mixed", "noise"], p=[0.6, 0.3, 0.1]))
    return w, h, scale, levels, nf, ini, mn, kind

def draw_crafted(rng):
    """Small images of all-tie or sparse structure; nfeatures from 1 (quotas of 0, below 4 * nIni)."""
    w = int(rng.integers(160, 700)); h = int(rng.integers(120, 400))
    scale = float(rng.choice([1.2, 1.5, 2.0]))
    w = max(w, h + 1)
    lmax = 1 + int(np.floor(np.log(min(w, h) / 64.0) / np.log(scale)))
    levels = int(rng.integers(1, max(2, min(8, lmax) + 1)))
    nf = int(rng.choice([1, 2, 3, 5, 8, 20, 50, 300, 2000]))
    ini = int(rng.integers(7, 30)); mn = int(rng.integers(2, ini + 1))
    kind = str(rng.choice(["lattice", "dots", "plateau"]))
    return w, h, scale, levels, nf, ini, mn, kind

def crafted_image(w, h, kind, rng):
    bg = int(rng.integers(0, 256))
    amp = int(rng.integers(1, 60)) * (1 if bg < 128 else -1)          # around the thresholds, both polarities
    y, x = np.mgrid[0:h, 0:w]
    if kind == "lattice":                                              # (x + mul * y + phase) % mod == 0: every response ties
        mod = int(rng.integers(5, 12)); mul = int(rng.integers(1, mod)); phase = int(rng.integers(0, mod))
        return np.where((x + mul * y + phase) % mod == 0, bg + amp, bg).astype(np.uint8)
    img = np.full((h, w), bg, np.int32)
    if kind == "dots":                                                 # sparse single pixels and adjacent pairs, a few amplitudes only: many ties
        n = int(rng.integers(1, 400))
        amps = rng.integers(1, 60, 4) * (1 if bg < 128 else -1)
        xs = rng.integers(0, w - 1, n); ys = rng.integers(0, h - 1, n); a = amps[rng.integers(0, 4, n)]
        img[ys, xs] = bg + a
        pair = rng.random(n) < 0.3
        img[ys[pair], xs[pair] + 1] = bg + a[pair]
    else:                                                              # plateaus: rectangles of one value, their corners tie in score
        for _ in range(int(rng.integers(1, 60))):
            x0 = int(rng.integers(0, w - 4)); y0 = int(rng.integers(0, h - 4))
            img[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 40))] = bg + amp
    return np.clip(img, 0, 255).astype(np.uint8)

def run(n_cases, seed0, crafted=False):
    pkg = g.load_package(); orc = g.load_oracle()
    fe, synth = pkg.frontend, pkg.synth
    rng = np.random.default_rng(seed0)
    ok = skipped = 0
    for k in range(n_cases):
        if crafted:
            w, h, scale, levels, nf, ini, mn, kind = draw_crafted(rng)
            img = crafted_image(w, h, kind, rng)
        else:
            w, h, scale, levels, nf, ini, mn, kind = draw(rng)
            img = synth.random_image(w, h, 1000 + k, kind)
        try:
            ex = fe.ORBextractor(nf, scale, levels, ini, mn)
            b = fe.Batch(ex, w, h, 1)
        except fe.SdError as e:
            skipped += 1
            print("case %d skipped (%s): %s" % (k, (w, h, scale, levels, nf), str(e)[:90]))
            continue
        b.extract_host(img[None])
        o = orc.Extractor(nf, scale, levels, ini, mn)
        rk, rd = o(img)
        kp, desc, per_level = b.download(0)
        same = np.array_equal(per_level, o.per_level) and kp.tobytes() == rk.tobytes() and np.array_equal(desc, rd)
        if crafted:
            same = same and np.array_equal(b.candidate_counts(0), o.cand_per_level)
        if not same:
            lv = [l for l in range(levels) if not np.array_equal(b.pyramid(0, l), o.pyramid(l))]
            print("MISMATCH case %d: %r  per-level %r vs %r; pyramid levels differing: %r" % (k, (w, h, scale, levels, nf, ini, mn, kind), per_level, o.per_level, lv))
            b.close()
            return 1
        ok += 1
        b.close()
    print("fuzz: %d cases identical, %d skipped as unsupported geometry" % (ok, skipped))
    return 0

if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--crafted"]
    sys.exit(run(int(args[0]) if args else 40, int(args[1]) if len(args) > 1 else 7, crafted="--crafted" in sys.argv[1:]))
