"""Static instruction counts of k_conv_f32's four instantiations (developer tool, also used by tests/test_conv_f32_isa_budget.py).

    python tools/conv_f32_isa_counts.py [--json]

Compiles tests/cpp/conv_f32_resources.hip to gfx950 assembly with the build's own flags and counts, per instantiation and per wave, in three
segments of the kernel's text -- before the first s_barrier (set-up and prologue), from the first to the last v_mfma (the K loop, with the
staging and the tap change inside it), after the last v_mfma (the four epilogue variants together):
  valu     vector ALU instructions (v_*, the MFMAs themselves not counted)
  imul     of those, the integer multiplies that run at quarter rate or slower (IMUL below)
  pk       of those, packed ones (v_pk_*)
  s_load   scalar loads (kernel arguments)
  s_wait   s_waitcnt
  branch   s_cbranch_* (exec-mask branches included)
The counts are of instructions in the text, not of instructions executed: a loop body counts once."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMUL = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mad_i64_i32", "v_mul_hi_i32")
TILES = ((16, 2, 2, 4), (16, 1, 2, 4), (16, 1, 1, 4), (8, 1, 1, 8))
SEGMENTS = ("before_first_barrier", "first_to_last_mfma", "after_last_mfma")
FIELDS = ("valu", "imul", "pk", "s_load", "s_wait", "branch")


def find_hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def assembly(hipcc, root=ROOT):
    """The device assembly of tests/cpp/conv_f32_resources.hip of the tree at `root`, compiled with that tree's build flags."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_graft_entry_for_isa_counts", os.path.join(root, "__graft_entry__.py"))
    graft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(graft)               # HIPCC_FLAGS and CSRC of the tree that is compiled
    flags = [f for f in graft.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory(prefix="conv_f32_isa_") as d:
        out = os.path.join(d, "conv_f32_resources.s")
        r = subprocess.run([hipcc] + flags + ["-I" + graft.CSRC, "--cuda-device-only", "-S", "-o", out,
                                              os.path.join(root, "tests", "cpp", "conv_f32_resources.hip")], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-4000:])
        with open(out) as f:
            return f.read()


def instructions(text, tile):
    """The mnemonics of one instantiation, in text order."""
    label = "_Z10k_conv_f32ILi%dELi%dELi%dELi%dEEv" % tile
    m = re.search(r"^%s\w*:" % re.escape(label), text, re.M)
    if not m:
        raise RuntimeError("k_conv_f32<%d, %d, %d, %d> is not in the assembly" % tile)
    end = text.index(".Lfunc_end", m.end())
    ops = []
    for line in text[m.end():end].splitlines():
        line = line.split(";")[0].strip()
        if not line or line.endswith(":") or line.startswith("."):
            continue
        ops.append(line.split()[0])
    return ops


def count(ops):
    def seg(part):
        valu = [o for o in part if o.startswith("v_") and not o.startswith("v_mfma")]
        return {"valu": len(valu), "imul": sum(o.startswith(IMUL) for o in valu), "pk": sum(o.startswith("v_pk_") for o in valu),
                "s_load": sum(o.startswith("s_load") for o in part), "s_wait": sum(o == "s_waitcnt" for o in part),
                "branch": sum(o.startswith("s_cbranch") for o in part)}
    bar = ops.index("s_barrier")
    mf = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
    return {"before_first_barrier": seg(ops[:bar]), "first_to_last_mfma": seg(ops[mf[0]:mf[-1] + 1]), "after_last_mfma": seg(ops[mf[-1] + 1:]),
            "mfma": len(mf)}


def counts(hipcc=None, root=ROOT):
    """{"16,2,2,4": {segment: {field: count}, "mfma": n}, ...} of the tree at `root`."""
    text = assembly(hipcc or find_hipcc(), root)
    return {",".join(str(v) for v in t): count(instructions(text, t)) for t in TILES}


def table(c):
    lines = ["%-12s %-22s %s" % ("tile", "segment", " ".join("%7s" % f for f in FIELDS))]
    for t, segs in c.items():
        for s in SEGMENTS:
            lines.append("%-12s %-22s %s" % ("<%s>" % t, s, " ".join("%7d" % segs[s][f] for f in FIELDS)))
        lines.append("%-12s %-22s %7d" % ("<%s>" % t, "v_mfma in the text", segs["mfma"]))
    return "\n".join(lines)


def main():
    root = ROOT
    args = [a for a in sys.argv[1:] if a != "--json"]
    if args:
        root = os.path.abspath(args[0])          # another checkout of this repository (the parent's, for the comparison)
    c = counts(root=root)
    print(json.dumps(c, indent=1) if "--json" in sys.argv else table(c))


if __name__ == "__main__":
    main()
