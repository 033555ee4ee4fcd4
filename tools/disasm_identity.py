"""Compare the gfx950 device code of every translation unit between two source trees (by default: the git revision REV, exported to a
temporary directory, and the working tree). Each unit of mppi-tf_amd/build.py UNITS is compiled device-only with the library's flags, the
code object is unbundled, every kernel symbol is disassembled (llvm-objdump -d; addresses, encodings, branch-target labels and comments
dropped) and its metadata notes (.vgpr_count, .sgpr_count, .agpr_count, LDS, scratch, spills) compared. Kernels that exist on one side
only are listed; a unit that exists on one side only is reported as new or gone.
    python tools/disasm_identity.py [--rev HEAD] [--jobs 8] [--keep DIR]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD", help="the 'before' git revision")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="a directory for the trees and code objects (default: a temporary one)")
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
    for stem in [u[2] for u in B.UNITS]:
        if stem not in cb:
            print("== %s: new unit, %d kernels: %s" % (stem, len(kernels(ca[stem])), sorted(kernels(ca[stem]))))
            continue
        if stem not in ca:
            print("== %s: unit gone" % stem)
            bad += 1
            continue
        kb, ka = kernels(cb[stem]), kernels(ca[stem])
        nb, na = notes(cb[stem]), notes(ca[stem])
        common = sorted(set(kb) & set(ka))
        same = [k for k in common if kb[k] == ka[k]]
        nsame = [k for k in common if nb.get(k) == na.get(k)]
        gone = sorted(set(kb) - set(ka))
        new = sorted(set(ka) - set(kb))
        bad += len(common) - len(same) + len(common) - len(nsame) + len(gone)
        print("== %s: kernels before %d, after %d, common %d, identical instructions %d, identical notes %d, only before: %s, only after: %s"
              % (stem, len(kb), len(ka), len(common), len(same), len(nsame), gone, new))
        for k in common:
            if kb[k] != ka[k] or nb.get(k) != na.get(k):
                print("   DIFFERS: %s (%d -> %d instructions; notes %s -> %s)" % (k, len(kb[k]), len(ka[k]), nb.get(k), na.get(k)))
    print("\n%s" % ("every existing kernel instance identical" if bad == 0 else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
