#!/usr/bin/env python3
"""Measures, on the CPU alone, what the OptimizeSim3 tests compare against (DESIGN Q45) and writes profiles/sim3_opt_tolerance.json:
per crafted case the decision margins of the sequential oracle and the spread of its values among its own variants (edges reversed,
-ffp-contract=fast where the host has FMA), and the LM margin: ten times the oracle's own flip distance, the largest rho / stop margin
at which one of those variants changes iterations / trials / stop, over the crafted cases and the fuzz's problems.  Never measured
against the device, and the kernel's summation order is not among the variants."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_opt_cases as sc  # noqa: E402


def main():
    out = {"chi2_margin_required": 1e-6, "value_factor": 10, "f32_ulps": 4, "fma_variant": sc.have_fma(), "cases": {}}
    flip = 0.0
    crafted = sc.crafted_cases()
    for c in crafted + [sc.random_problem(k) for k in range(300)]:
        r, st, info, mg = sc.solve(c)
        sp = sc.spread(c)
        if sp["lm_counts_differ"] and c.get("sane", True):
            flip = max(flip, sc.lm_margin_of(mg))
        if c in crafted:
            out["cases"][c["name"]] = {"chi2_margin": float(mg[sc.M_CHI2]), "rho_margin": float(mg[sc.M_RHO]), "stop_margin": float(mg[sc.M_STOP]),
                                       "spread": {f: sp[f] for f in sc.VALUE_FIELDS}, "lm_counts_differ": sp["lm_counts_differ"]}
    out["lm_flip_distance"] = flip
    out["lm_margin"] = 10 * flip
    for c in crafted:
        v = out["cases"][c["name"]]
        v["lm_held"] = int(c.get("sane", True) and min(v["rho_margin"], v["stop_margin"]) >= out["lm_margin"])
    big = 1.7e308
    for v in out["cases"].values():
        for k in ("chi2_margin", "rho_margin", "stop_margin"):
            if v[k] > big:
                v[k] = None                                  # no such decision was taken
        for f in sc.VALUE_FIELDS:
            if v["spread"][f] != v["spread"][f]:
                v["spread"][f] = None                        # NaN values: compared as NaN
    path = os.path.join(ROOT, "profiles", "sim3_opt_tolerance.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(v["lm_counts_differ"] for v in out["cases"].values())
    print("LM flip distance %.3g, %d cases held to the sequential LM counts" % (out["lm_flip_distance"], sum(v["lm_held"] for v in out["cases"].values())))
    print("%d cases; LM counts change with the summation order in %d; smallest chi2 margin %.3g; largest spread %.3g" % (
        len(out["cases"]), n, min(v["chi2_margin"] for v in out["cases"].values() if v["chi2_margin"] is not None),
        max(max(x for x in v["spread"].values() if x is not None) for v in out["cases"].values() if any(x is not None for x in v["spread"].values()))))


if __name__ == "__main__":
    main()
