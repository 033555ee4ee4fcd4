#!/usr/bin/env python3
"""Vector instructions and priced issue cycles of the producers' horizon-loop slots of ONE k_rollout_pc instance, from hipcc -S output:
   tools/static_slot_price.py <before.s> <after.s> [mangled-name-substring]
The kernel's text is cut at its s_barrier instructions: a producer slot (one horizon group of one producer wave: nominal actions, Philox,
Box-Muller, scale, action cost, LDS slots) is the text between two chunk barriers, and the slots of the horizon loop are the segments whose
vector instructions include Philox products: two copies, of which the one with fewer vector instructions per slot is the C++ action-cost
form that BASELINE runs (hipcc lays the gamma / upsilon copy out first; until r06 this tool priced that one). Blocks the compiler moved out of line (the rolled
Philox of a launch whose block indices straddle 2^32) lie behind the last barrier and are not part of any slot. Each opcode is classed as
tools/valu_static_mix.py classes it and priced as tools/summarize_profiles.py prices the class (profiles/r02_valu_issue.json, four waves per
SIMD). `per tile` = 16 slots (H = 64: 16 horizon groups, whichever producer draws them)."""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from valu_static_mix import classify  # noqa: E402

cyc = {r["op"]: r["cyc_per_inst_per_simd"] for r in json.load(open(os.path.join(ROOT, "profiles", "r02_valu_issue.json")))
       if r["waves_per_simd_median"] == 4}
PRICE = {"add_f32": cyc["v_add_f32"], "mul_f32": cyc["v_mul_f32"], "fma_f32": cyc["v_fma_f32"],
         "trans_f32": (cyc["v_log_f32"] + cyc["v_sqrt_f32"] + cyc["v_sin_f32"]) / 3, "int32": cyc["v_xor_b32"], "int64": cyc["v_mad_u64_u32 (+0)"],
         "cvt": cyc["v_cvt_f32_u32"], "pk_add_f32": cyc["v_pk_add_f32"], "pk_mul_f32": cyc["v_pk_mul_f32"], "pk_fma_f32": cyc["v_pk_fma_f32"],
         "other:mov": cyc["v_mov_b32"], "other:bitop3": cyc["v_bitop3_b32"], "other:dpp_f32": cyc["v_add_f32_dpp quad_perm"],
         "other:dpp_mov": cyc["v_mov_b32_dpp row_mirror"], "other:permlane_swap": cyc["v_mov_b32_dpp row_mirror"],
         "other:cndmask": cyc["v_cndmask_b32_e64 (mask in s[44:45])"], "other:lane": cyc["v_readlane_b32"], "other:minmax": cyc["v_max_f32"],
         "other:cmp": cyc["v_xor_b32"], "other:bitfield3": cyc["v_bitop3_b32"], "other:misc": cyc["v_bitop3_b32"]}


def kernel_text(path, pat):
    lines = open(path).read().split("\n")
    st = next(i for i, l in enumerate(lines) if pat in l and l.split(";")[0].strip().endswith(":") and not l.startswith((".", "\t")))
    end = next(i for i in range(st, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return [l.split(";")[0].strip() for l in lines[st + 1:end]]


def segments(text):
    seg, cur = [], []
    for l in text:
        if not l or l[0] == "." or l.endswith(":"):
            continue
        op = l.split()[0]
        if op == "s_barrier":
            seg.append(cur)
            cur = []
        else:
            cur.append(op)
    seg.append(cur)
    return seg


def tally(ops):
    cls, opc = collections.Counter(), collections.Counter()
    for op in ops:
        if op.startswith("v_"):
            cls[classify(op)] += 1
            opc[re.sub(r"_e(32|64)$", "", op)] += 1
    return cls, opc


def main():
    pat = sys.argv[3] if len(sys.argv) > 3 else "k_rollout_pcILi3ELi3ELi6ELb1ELi0ELi0E"
    res, copy_note = [], []
    for path in sys.argv[1:3]:
        segs = segments(kernel_text(path, pat))
        slots = [s for s in segs if sum(1 for op in s if op.startswith("v_mad_u64_u32")) >= 40]
        # two copies of the horizon loop, NSLOT slots each, in whichever order hipcc lays them out (it has put the gamma / upsilon form in
        # front of the C++ form the source names first). The C++ action-cost form is the one BASELINE runs: the copy with fewer vector
        # instructions per slot — the gamma / upsilon form computes everything it does plus the u and u.eps terms of every action.
        half = len(slots) // 2
        copies = [slots[:half], slots[half:]] if half else [slots]
        nvec = [sorted(sum(1 for op in s if op.startswith("v_")) for s in c)[len(c) // 2] for c in copies]
        cpp = copies[nvec.index(min(nvec))]
        copy_note.append("%s: copies of the horizon loop in text order, vector instructions of their median slot: %s -> priced: the %d-instruction copy"
                         % (os.path.basename(path), ", ".join(str(n) for n in nvec), min(nvec)))
        # slots 1..5 of that copy (slot 0 of the copy in front shares its segment with the kernel's head; the copy behind has no such slot,
        # its first five full slots are taken all the same so that the columns line up)
        first = cpp[1:6] if cpp is copies[0] else cpp[0:5]
        tallies = [tally(s) for s in first]
        ref = tallies[1]
        whole = tally([op for s in segs for op in s])
        res.append(dict(path=path, n_slots=len(slots), per_slot=[(sum(c.values()), sum(n * PRICE[k] for k, n in c.items()), sum(1 for op in s if op.startswith("s_")))
                                                               for (c, _), s in zip(tallies, first)],
                        cls=ref[0], opc=ref[1], whole=whole[0]))
    b, a = res
    print("k_rollout_pc<3, 3, 6, true, 0, 0>: static vector-instruction mix of a producer slot (slot 2 of the C++ action-cost copy of the horizon loop)")
    print("prices: cycles per instruction per SIMD at four waves per SIMD, profiles/r02_valu_issue.json, classes as tools/summarize_profiles.py")
    print("\n".join(copy_note) + "\n")
    print("%-22s %8s %8s %10s %10s %10s" % ("class", "before", "after", "price", "cyc before", "cyc after"))
    for k in sorted(set(b["cls"]) | set(a["cls"])):
        print("%-22s %8d %8d %10.3f %10.1f %10.1f" % (k, b["cls"][k], a["cls"][k], PRICE[k], b["cls"][k] * PRICE[k], a["cls"][k] * PRICE[k]))
    tb, ta = sum(b["cls"].values()), sum(a["cls"].values())
    cb, ca = sum(n * PRICE[k] for k, n in b["cls"].items()), sum(n * PRICE[k] for k, n in a["cls"].items())
    print("%-22s %8d %8d %10s %10.1f %10.1f" % ("slot total", tb, ta, "", cb, ca))
    print("%-22s %8d %8d %10s %10.1f %10.1f   (16 slots: the horizon loop of one tile's three producers)" % ("tile total", 16 * tb, 16 * ta, "", 16 * cb, 16 * ca))
    print("\nopcodes of the slot (before -> after):")
    for k in sorted(set(b["opc"]) | set(a["opc"]), key=lambda k: -b["opc"][k]):
        print("  %-28s %4d -> %4d%s" % (k, b["opc"][k], a["opc"][k], "" if b["opc"][k] == a["opc"][k] else "   *"))
    print("\nslots 1..5 one by one (vector instructions, priced cycles, scalar instructions):")
    for name, r in (("before", b), ("after", a)):
        print("  %-7s %s" % (name, "  ".join("%d / %.0f / %d" % t for t in r["per_slot"])))
    print("\nwhole kernel, static (both copies of the horizon loop, head, weighted sums, consumer, out-of-line blocks):")
    for k in sorted(set(b["whole"]) | set(a["whole"])):
        print("  %-22s %6d -> %6d" % (k, b["whole"][k], a["whole"][k]))


if __name__ == "__main__":
    main()
