#!/usr/bin/env python3
"""Random OptimizeSim3 problems (tests/sim3_opt_cases.random_problem: 20 - 300 correspondences, outliers in either image, either
scale mode, seeds 0 .. n-1) through the CPU oracle and, with --gpu, through sd_sim3_optimize_host; profiles/sim3_opt_fuzz.json.
A problem one of whose chi2 decisions lies inside the relative margin of profiles/sim3_opt_tolerance.json is skipped and counted; at
most 5 % may be (a condition on the seeds, which the oracle alone must meet: tests/test_sim3_opt_oracle.py asserts it).  The others
are held to DESIGN Q45: bit for bit against the oracle in the kernel's summation order, and against the sequential oracle the chi2
decisions equal, the values within max(10 x spread, 4 f32 ulps), and iterations / trials / stop equal for every problem whose LM
decisions lie outside the LM margin (ten times the oracle's own flip distance); how many problems that leaves is reported, not capped:
a converged problem's LM decisions are rounding noise in the oracle itself."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_opt_cases as sc  # noqa: E402

MAX_SKIPPED = 0.05


def oracle_pass(n, margin):
    """(cases, packed tables, sequential results, wave results, skipped mask, per-field spread (n,))."""
    cases = [sc.random_problem(k) for k in range(n)]
    off, corr, probs = sc.pack(cases)
    seq = sc.solve_packed(off, corr, probs, 0, 16)
    wave = sc.solve_packed(off, corr, probs, sc.WAVE, 16)
    rev = sc.solve_packed(off, corr, probs, sc.REVERSE, 16)
    runs = [rev] + ([sc.solve_packed(off, corr, probs, 0, 16, "fast")] if sc.have_fma() else [])       # the spread's variants: not the kernel's order
    skipped = seq[3][:, sc.M_CHI2] < margin
    spread = {f: np.max([np.abs(r[0][f].astype(np.float64) - seq[0][f].astype(np.float64)).reshape(n, -1).max(1) for r in runs], 0) for f in sc.VALUE_FIELDS}
    flips = sum(int((r[0]["ret"] != seq[0]["ret"]).sum() + (r[0]["n_bad"] != seq[0]["n_bad"]).sum()) for r in runs)
    return cases, (off, corr, probs), seq, wave, skipped, spread, flips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=300)
    ap.add_argument("--gpu", action="store_true", help="also run the device and compare")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_opt_fuzz.json"))
    a = ap.parse_args()
    with open(os.path.join(ROOT, "profiles", "sim3_opt_tolerance.json")) as f:
        tol = json.load(f)
    cases, (off, corr, probs), seq, wave, skipped, spread, flips = oracle_pass(a.problems, tol["chi2_margin_required"])
    lm_margin = tol["lm_margin"]
    lm_held = np.minimum(seq[3][:, sc.M_RHO], seq[3][:, sc.M_STOP]) >= lm_margin
    for r in (wave[0], sc.solve_packed(off, corr, probs, sc.REVERSE, 16)[0]):        # outside the margin no variant changes a counter
        assert all(sc.lm_counts(r[i]) == sc.lm_counts(seq[0][i]) for i in np.nonzero(lm_held)[0])
    rec = dict(tool="fuzz_sim3_opt", problems=a.problems, skipped=int(skipped.sum()), max_skipped=MAX_SKIPPED,
               smallest_chi2_margin=float(seq[3][:, sc.M_CHI2].min()), chi2_decisions_changed_by_an_oracle_variant=flips,
               lm_counts_changed_by_the_kernels_order=int(sum(seq[0][k][i].tolist() != wave[0][k][i].tolist() for i in range(a.problems)
                                                              for k in ("trials",))),
               largest_spread={f: float(spread[f].max()) for f in sc.VALUE_FIELDS}, matched=int((seq[0]["ret"] >= 20).sum()),
               returned_zero=int((seq[0]["written"] == 0).sum()), lm_margin=lm_margin,
               lm_decisions_outside_the_margin=int(lm_held.sum()), device=None)
    assert rec["skipped"] <= MAX_SKIPPED * a.problems, rec
    if a.gpu:
        import __graft_entry__ as g
        fe = g.load_package().frontend
        res, st = fe.sim3_optimize(off, corr, probs)
        bit = int(sum(res[i].tobytes() == wave[0][i].tobytes() for i in range(a.problems)))
        worst, decisions = 0.0, 0
        for i in range(a.problems):
            if skipped[i]:
                continue
            d, r = res[i], seq[0][i]
            decisions += int((d["ret"], d["n_bad"], d["more_iterations"], d["written"]) != (r["ret"], r["n_bad"], r["more_iterations"], r["written"]))
            decisions += int(st[off[i]:off[i + 1]].tobytes() != seq[1][off[i]:off[i + 1]].tobytes())
            decisions += int(bool(lm_held[i]) and sc.lm_counts(d) != sc.lm_counts(r))
            for f in sc.VALUE_FIELDS:
                x, y = np.asarray(d[f], np.float64), np.asarray(r[f], np.float64)
                bound = np.maximum(tol["value_factor"] * spread[f][i], tol["f32_ulps"] * 2.0 ** -23 * np.abs(y))
                worst = max(worst, float((np.abs(x - y) / np.maximum(bound, 1e-300)).max()))
        rec["device"] = dict(bit_identical_to_the_oracle_in_kernel_order=bit, state_identical=bool(st.tobytes() == wave[1].tobytes()),
                             decisions_differing_from_the_sequential_oracle=decisions, worst_value_error_over_bound=worst)
        assert bit == a.problems and rec["device"]["state_identical"] and decisions == 0 and worst <= 1.0, rec
    # a dozen scenes through the whole refine chain, free-running on the CPU; with --gpu on the device, stage by stage
    import sim3_refine_cases as rc
    import triangulate_cases as tc
    scenes = [rc.refine_scene(100 + k, (300, 120, 60)[k % 3], 2 + k % 3, not_found=((1,) if k % 4 == 0 else ()), noise=(0.7, 2.0)[k % 2]) for k in range(12)]
    jobs = [j for sc_ in scenes for j in rc.cpu_refine(sc_, tc.Levels(), 4096, fix_scale=False)]
    rec["scenes"] = dict(scenes=len(scenes), jobs=len(jobs), not_run=sum(1 - j["ran"] for j in jobs), matched=sum(j["ret"] >= 20 for j in jobs),
                         below_the_gate=sum(j["ran"] and j["ret"] < 20 for j in jobs), added=sum(j["added"] for j in jobs),
                         added_then_removed=sum(j["added_then_removed"] for j in jobs), not_in_kf2=sum(j["minus2"] for j in jobs), device=None)
    if a.gpu:
        import fuse_cases as fc
        pkg = g.load_package()
        ws = fc.Workspace(pkg.frontend, 8, tc.vocabulary(pkg.synth, 5))
        n = 0
        for sc_ in scenes:
            got, seen = rc.check_refine(ws, sc_)
            n += len(got)
        ws.close()
        rec["scenes"]["device"] = dict(jobs_compared_stage_by_stage=n, mismatches=0)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
