#!/usr/bin/env python3
"""Static counts of a finish kernel from its gfx950 assembly (profiles/finish_static.txt):
   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I include --cuda-device-only -S mppi-tf_amd/csrc/mppi_capi_step.hip -o step.s
   python tools/finish_static.py step.s KERNEL_SUBSTRING [--skip BLOCK,BLOCK,...]
Splits the kernel into its basic blocks (the entry is `bb.0`, then `bb.N` / `LBBx_y` as hipcc names them) and prints, per block, the
instructions, the vector instructions (v_*) and the s_waitcnt; then two sums over the blocks that are NOT skipped, in text order:
  head: everything in front of the first global_load_dword that is not an `sc1` load (the first record load),
  all : the whole path (thread 0's, when the skipped blocks are those it does not execute).
Which blocks a launch skips is read off the branches by hand and passed with --skip; the file under profiles/ lists them."""
import re
import sys


def blocks_of(path, needle):
    out, cur, inside = [], None, False
    for line in open(path):
        s = line.strip()
        if not inside:
            if re.match(r"^_Z\w*:", line) and needle in line.split(":")[0]:
                inside, cur = True, ["bb.0", []]
                out.append(cur)
            continue
        if s.startswith(".section") or s.startswith(".Lfunc_end"):
            break
        lab = re.match(r"^; %(bb\.\d+):", s) or re.match(r"^\.(LBB\d+_\d+):", s)
        if lab and lab.group(1) == "bb.0":
            continue
        if lab:
            cur = [lab.group(1), []]
            out.append(cur)
        elif s and not s.startswith(";") and not s.startswith("."):
            cur[1].append(s)
    return out


def main():
    path, needle = sys.argv[1], sys.argv[2]
    skip = set(sys.argv[sys.argv.index("--skip") + 1].split(",")) if "--skip" in sys.argv else set()
    head, total, in_head = [0, 0, 0], [0, 0, 0], True
    print("%-10s %6s %6s %8s" % ("block", "instr", "v_*", "waitcnt"))
    for name, ins in blocks_of(path, needle):
        n = (len(ins), sum(i.startswith("v_") for i in ins), sum(i.startswith("s_waitcnt") for i in ins))
        print("%-10s %6d %6d %8d%s" % (name, *n, "   (skipped)" if name in skip else ""))
        if name in skip:
            continue
        for i in ins:
            if in_head and i.startswith("global_load_dword") and "sc1" not in i:
                in_head = False
            for acc in ([head] if in_head else []) + [total]:
                acc[0] += 1
                acc[1] += i.startswith("v_")
                acc[2] += i.startswith("s_waitcnt")
    print("head (in front of the first record load): %d instructions, %d vector, %d s_waitcnt" % tuple(head))
    print("all (entry to s_endpgm on this path)    : %d instructions, %d vector, %d s_waitcnt" % tuple(total))


if __name__ == "__main__":
    main()
