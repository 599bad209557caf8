#!/usr/bin/env python3
"""Writes tests/golden/dbow2_ref.npz: what the reference's DBoW2 BowVector / FeatureVector (oracle/_ref/libdbow2_ref.so, built by
__graft_entry__.build() where the reference tree is mounted) returns for the inputs of tests/test_oracle_dbow2_ref.py.

  python tools/gen_dbow2_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import test_oracle_dbow2_ref as t  # noqa: E402

if not os.path.exists(t.REF_SO):
    raise SystemExit("%s is not built: run __graft_entry__.build() where the reference tree is mounted" % t.REF_SO)
ref = C.CDLL(t.REF_SO)
orc, synth = graft.load_oracle(), graft.load_package().synth
out = {}
for case in t.CASES:
    _, _, word, weight, node = t.case_inputs(orc, synth, *case)
    key = t.case_key(*case)
    for f, a in zip(("word", "weight", "node"), (word, weight, node)):
        out[key + "_" + f] = np.asarray(a).copy()
    for f, a in zip(("bw", "bv", "fn", "ff"), t._ref_bow(ref, word, weight, node)):
        out[key + "_" + f] = a
out["add_if_not_exist_bw"], out["add_if_not_exist_bv"] = t.ref_add_if_not_exist(ref)
np.savez_compressed(t.GOLDEN, **out)
print("wrote", os.path.relpath(t.GOLDEN, ROOT), sum(a.nbytes for a in out.values()), "bytes before compression")
