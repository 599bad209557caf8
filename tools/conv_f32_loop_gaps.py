"""What sits between the MFMAs of k_conv_f32's K steps in the compiler's output (developer tool, also used by
tests/test_conv_f32_loop_schedule.py).

    python tools/conv_f32_loop_gaps.py [--loop | --json] [checkout]

Compiles tests/cpp/conv_f32_resources.hip as tools/conv_f32_isa_counts.py does (its assembly() and instructions()) and prints, per instantiation
and per K step in the text (the loop holds two, one per LDS buffer, a third follows it for an odd step count), every gap between two consecutive
v_mfma with its instructions by class:
  vmem      global / buffer / flat / scratch loads and stores
  ds_read, ds_write
  valu      every other v_* instruction
  salu      s_* other than waits, branches and the barrier
  wait      s_waitcnt (with its counters) and s_nop
  branch    s_cbranch_* / s_branch
A step is the text from one s_barrier to the next that holds MFMAs; an MFMA gap costs the SIMD about max(the MFMA's 64 cycles, the issue costs of
what stands in it), so what matters is that no gap collects the step's staging.  --loop prints the steps' instructions themselves (what
profiles/conv_f32_schedule_isa.txt records); --json prints step_counts(), the per-step instruction counts by class that
tests/golden/conv_f32_walk_parent.json records of a parent commit; `checkout` names another tree of this repository (the parent's, for the
comparison)."""
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("vmem", "ds_read", "ds_write", "valu", "salu", "wait", "branch")


def _counts_tool():
    spec = importlib.util.spec_from_file_location("sd_conv_f32_isa_counts", os.path.join(ROOT, "tools", "conv_f32_isa_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _counts_tool()
TILES = TOOL.TILES


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_"):
        return "ds_write"
    if op.startswith("v_"):
        return "valu"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op == "s_barrier":
        return "barrier"
    return "salu"


def body(text, tile):
    """[(mnemonic, operands)] of one instantiation in text order: the lines TOOL.instructions() keeps, with their operands."""
    label = "_Z10k_conv_f32ILi%dELi%dELi%dELi%dEEv" % tile
    m = re.search(r"^%s\w*:" % re.escape(label), text, re.M)
    if not m:
        raise RuntimeError("k_conv_f32<%d, %d, %d, %d> is not in the assembly" % tile)
    end = text.index(".Lfunc_end", m.end())
    out = []
    for line in text[m.end():end].splitlines():
        line = line.split(";")[0].strip()
        if not line or line.endswith(":") or line.startswith("."):
            continue
        parts = line.split(None, 1)
        out.append((parts[0], parts[1] if len(parts) > 1 else ""))
    assert [o for o, _ in out] == TOOL.instructions(text, tile)
    return out


class Step(list):
    """The gaps of one K step, gap g = the instructions between MFMA g - 1 and MFMA g (gap 0: from the barrier in front of the step to its first
    MFMA; in the text that can include blocks that do not belong to the step); .tail: from its last MFMA to the barrier behind it."""
    tail = ()


def steps(ins):
    """The K steps of one instantiation, in text order."""
    out, cur, gap = [], None, []
    for op, args in ins:
        c = classify(op)
        if c == "barrier":
            if cur:
                cur.tail = gap
                out.append(cur)
            cur, gap = Step(), []
        elif cur is None:
            continue
        elif c == "mfma":
            cur.append(gap)
            gap = []
        else:
            gap.append((op, args))
    return out


def gap_counts(gap):
    c = dict.fromkeys(CLASSES, 0)
    for op, _ in gap:
        c[classify(op)] += 1
    return c


def vmcnt_waits(step):
    """The N of every s_waitcnt vmcnt(N) from a step's first MFMA to the barrier behind it."""
    out = []
    for gap in step[1:] + [step.tail]:
        for op, args in gap:
            m = re.search(r"vmcnt\((\d+)\)", args) if op == "s_waitcnt" else None
            if m:
                out.append(int(m.group(1)))
    return out


def metadata(text, tile):
    """{"vgpr_count", "private_segment_fixed_size", "waves_per_simd"} from the kernel's metadata record."""
    name = "_Z10k_conv_f32ILi%dELi%dELi%dELi%dEEv11SdConvArgsF" % tile
    at = text.index(".name:           " + name)
    rec = text[at:text.index(".wavefront_size", at)]
    md = {k: int(re.search(r"\.%s:\s+(\d+)" % k, rec).group(1)) for k in ("vgpr_count", "private_segment_fixed_size")}
    md["waves_per_simd"] = min(8, 512 // ((md["vgpr_count"] + 7) // 8 * 8))      # 512 registers per SIMD lane, allocated in eights
    return md


def loop_part(step):
    """The instructions of a step from its first MFMA to the barrier behind it, tap-change block included: every gap but gap 0 (which, for the
    first step in the text, also holds blocks in front of the loop), and the tail."""
    return [ins for gap in step[1:] for ins in gap] + list(step.tail)


def staging_loads(step):
    """[(mnemonic, destination, address VGPR or None)] of the vector-memory instructions of loop_part(step).  A buffer load's address register
    is its voffset (`buffer_load_dwordx4 v[a:b], vN, s[c:d], sK offen`), a global load's the 64-bit pair."""
    out = []
    for op, args in loop_part(step):
        if classify(op) == "vmem":
            f = [a.strip() for a in args.split(",")]
            out.append((op, f[0], f[1] if len(f) > 1 and f[1].startswith("v") else None))
    return out


def valu_writes(gap, reg):
    """The VALU instructions of `gap` whose destination overlaps VGPR `reg` ("v107", or a pair "v[106:107]")."""
    r = re.fullmatch(r"v\[(\d+):(\d+)\]", reg)
    first, last = (int(r.group(1)), int(r.group(2))) if r else (int(reg[1:]),) * 2      # a global load's address is a register pair
    hits = []
    for op, args in gap:
        if classify(op) != "valu":
            continue
        dst = args.split(",")[0].strip()
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", dst)
        lo, hi = (int(m.group(1)), int(m.group(2))) if m else ((int(dst[1:]),) * 2 if re.fullmatch(r"v\d+", dst) else (-1, -1))
        if lo <= last and first <= hi:
            hits.append((op, args))
    return hits


def step_counts(text):
    """{"16,2,2,4": [per step in the text {"loop": counts by class of loop_part(step), "whole": the same with gap 0}], ...}"""
    out = {}
    for tile in TILES:
        rows = []
        for st in steps(body(text, tile)):
            loop = gap_counts(loop_part(st))
            whole = gap_counts(list(st[0]) + loop_part(st))
            rows.append({"mfma": len(st), "loop": loop, "whole": whole})
        out[",".join(str(v) for v in tile)] = rows
    return out


def _line(where, gap):
    c = gap_counts(gap)
    return "    %-14s %s%s" % (where, "  ".join("%s %d" % (k, c[k]) for k in CLASSES if c[k]), "   [%s]" % ", ".join(a for o, a in gap if o == "s_waitcnt") if c["wait"] else "")


def report(text, loop=False):
    lines = []
    for tile in TILES:
        ins = body(text, tile)
        md = metadata(text, tile)
        lines.append("k_conv_f32<%d, %d, %d, %d>: %d VGPRs, %d waves per SIMD, private segment %d bytes" % (tile + (md["vgpr_count"], md["waves_per_simd"], md["private_segment_fixed_size"])))
        for si, st in enumerate(steps(ins)):
            lines.append("  step %d: %d MFMAs, vmcnt waits %s" % (si, len(st), vmcnt_waits(st)))
            for g, gap in enumerate(st):
                c = gap_counts(gap)
                if loop:
                    lines.append("    -- %s" % ("before MFMA 0" if g == 0 else "behind MFMA %d" % (g - 1)))
                    lines += ["       %s %s" % (op, args) for op, args in gap]
                elif gap:
                    lines.append(_line("before MFMA 0" if g == 0 else "behind MFMA %d" % (g - 1), gap))
            if loop:
                lines.append("    -- behind MFMA %d, to the barrier" % (len(st) - 1))
                lines += ["       %s %s" % (op, args) for op, args in st.tail]
            else:
                lines.append(_line("behind MFMA %d" % (len(st) - 1), st.tail))
    return "\n".join(lines)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    root = os.path.abspath(args[0]) if args else ROOT
    text = TOOL.assembly(TOOL.find_hipcc(), root)
    if "--json" in sys.argv:
        import json
        print(json.dumps(step_counts(text), indent=1))
    else:
        print(report(text, "--loop" in sys.argv))


if __name__ == "__main__":
    main()
