"""Compare the gfx950 device code of every translation unit between two source trees (by default: the git revision REV, exported to a
temporary directory, and the working tree). Each unit of mppi-tf_amd/build.py UNITS is compiled device-only with the library's flags, the
code object is unbundled, every kernel symbol is disassembled (llvm-objdump -d; addresses, encodings, branch-target labels and comments
dropped) and its metadata notes (.vgpr_count, .sgpr_count, .agpr_count, LDS, scratch, spills) compared. Kernels that exist on one side
only are listed; a unit that exists on one side only is reported as new or gone. The units of one group (--union STEM: the stem itself and
every STEM_*; by default the C-ABI units, capi) are compared as the union of their kernels by symbol, so a kernel may change units within
the group; a kernel that the working tree defines in more than one unit, and did not before, is reported and counts as a difference.
    python tools/disasm_identity.py [--rev HEAD] [--jobs 8] [--keep DIR] [--union capi]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mppi-tf_amd"))
import build as B  # noqa: E402

LLVM = "/opt/rocm/llvm/bin"
NOTE_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".sgpr_spill_count", ".vgpr_spill_count")


def units(tree):
    """(stem, cmd-args) of every unit whose source exists in `tree`: the build's UNITS plus any unit that exists only there"""
    out = []
    for src, defs, stem in B.UNITS:
        path = os.path.join(tree, "mppi-tf_amd", "csrc", src)
        if os.path.exists(path):
            mlp = stem.startswith("mlp_") or stem in B.MLP_STEMS
            out.append((stem, [*(B.MLP_FLAGS + B.MLP_ONLY_FLAGS if mlp else []), *["-D" + d for d in defs], path]))
    return out


def compile_tree(tree, outdir, jobs):
    os.makedirs(outdir, exist_ok=True)

    def one(u):
        stem, args = u
        co = os.path.join(outdir, stem + ".co")
        flags = ["-O3", "--offload-arch=" + B.ARCH, "-ffp-contract=off", "-std=c++17", "-fPIC", "-I", os.path.join(tree, "include")]
        subprocess.check_call([B.hipcc(), *flags, "--cuda-device-only", "-c", *args, "-o", co + ".bundle"])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + co + ".bundle",
                               "--targets=hipv4-amdgcn-amd-amdhsa--" + B.ARCH, "--output=" + co])
        return stem, co

    with ThreadPoolExecutor(jobs) as pool:
        return dict(pool.map(one, units(tree)))


def kernels(co):
    """{kernel symbol: [instructions]} of one code object"""
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or not line.strip() or line.startswith("Disassembly"):
            continue
        ins = re.sub(r"\s*(//|;).*$", "", line).strip()
        ins = re.sub(r"<[^>]*>", "", ins).strip()
        if ins:
            out[cur].append(re.sub(r"\s+", " ", ins))
    # the padding behind a kernel's last instruction (alignment; the instruction-prefetch pad at the end of the code object) belongs to
    # the kernel's place in its unit, not to the kernel: a kernel that changes units keeps its instructions and not its padding
    for v in out.values():
        while v and (v[-1].startswith("s_nop") or v[-1] == "s_code_end"):
            v.pop()
    return {k: v for k, v in out.items() if not k.endswith(".kd")}


def notes(co):
    """{kernel symbol: (metadata values)}"""
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for block in re.split(r"\n\s*- \.", txt)[1:]:
        kv = dict(re.findall(r"^\s*-?\s*(\.[a-z_]+):\s*(\S+)", "." + block, re.M))
        name = kv.get(".name")
        if name:
            out[name] = tuple(kv.get(k) for k in NOTE_KEYS)
    return out


def compare(tag, kb, ka, nb, na):
    """print one comparison line (and every kernel that differs); the number of differences"""
    common = sorted(set(kb) & set(ka))
    same = [k for k in common if kb[k] == ka[k]]
    nsame = [k for k in common if nb.get(k) == na.get(k)]
    gone = sorted(set(kb) - set(ka))
    new = sorted(set(ka) - set(kb))
    print("== %s: kernels before %d, after %d, common %d, identical instructions %d, identical notes %d, only before: %s, only after: %s"
          % (tag, len(kb), len(ka), len(common), len(same), len(nsame), gone, new))
    for k in common:
        if kb[k] != ka[k] or nb.get(k) != na.get(k):
            print("   DIFFERS: %s (%d -> %d instructions; notes %s -> %s)" % (k, len(kb[k]), len(ka[k]), nb.get(k), na.get(k)))
    return len(common) - len(same) + len(common) - len(nsame) + len(gone)


def owners(cos):
    """{kernel symbol: [stems that define it]} over the code objects {stem: path}"""
    out = {}
    for stem in sorted(cos):
        for k in kernels(cos[stem]):
            out.setdefault(k, []).append(stem)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD", help="the 'before' git revision")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="a directory for the trees and code objects (default: a temporary one)")
    ap.add_argument("--union", default="capi", help="stem of the unit group compared as a union by kernel symbol (STEM and STEM_*)")
    o = ap.parse_args()
    work = o.keep or tempfile.mkdtemp(prefix="disasm_identity_")
    before = os.path.join(work, "before_src")
    os.makedirs(before, exist_ok=True)
    subprocess.check_call("git -C %s archive %s | tar -x -C %s" % (ROOT, o.rev, before), shell=True)
    cb = compile_tree(before, os.path.join(work, "before"), o.jobs)
    ca = compile_tree(ROOT, os.path.join(work, "after"), o.jobs)
    print("Existing kernel instances before (%s) and after (the working tree), gfx950 device code of each translation unit" % o.rev)
    print("(hipcc -O3 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only with each unit's flags, unbundled, llvm-objdump -d per kernel")
    print("symbol; addresses, encodings, branch-target labels and comments dropped). Kernel metadata (%s) from llvm-readelf --notes.\n"
          % ", ".join(NOTE_KEYS))
    bad = 0
    in_union = lambda stem: stem == o.union or stem.startswith(o.union + "_")  # noqa: E731
    for stem in [u[2] for u in B.UNITS]:
        if in_union(stem):
            continue
        if stem not in cb:
            print("== %s: new unit, %d kernels: %s" % (stem, len(kernels(ca[stem])), sorted(kernels(ca[stem]))))
            continue
        if stem not in ca:
            print("== %s: unit gone" % stem)
            bad += 1
            continue
        bad += compare(stem, kernels(cb[stem]), kernels(ca[stem]), notes(cb[stem]), notes(ca[stem]))
    # the union group: every kernel of its units by symbol, whichever unit holds it
    kb, ka, nb, na = {}, {}, {}, {}
    for cos, ks, ns in ((cb, kb, nb), (ca, ka, na)):
        for stem in sorted(cos):
            if in_union(stem):
                ks.update(kernels(cos[stem]))
                ns.update(notes(cos[stem]))
    stems = lambda cos: " + ".join(sorted(x for x in cos if in_union(x)))  # noqa: E731
    bad += compare("union of %s (before: %s)" % (stems(ca), stems(cb)), kb, ka, nb, na)
    for stem in sorted(x for x in ca if in_union(x)):
        print("   %s: %d kernels: %s" % (stem, len(kernels(ca[stem])), sorted(kernels(ca[stem]))))
    ob, oa = owners(cb), owners(ca)
    dup = {k: v for k, v in oa.items() if len(v) > 1}
    new_dup = {k: v for k, v in dup.items() if len(ob.get(k, [])) <= 1}
    bad += len(new_dup)
    print("kernels defined in more than one unit of the working tree: %d (%d of them in one unit at most before)" % (len(dup), len(new_dup)))
    for k, v in sorted(new_dup.items()):
        print("   DUPLICATE: %s in %s" % (k, ", ".join(v)))
    print("\n%s" % ("every existing kernel instance identical" if bad == 0 else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
