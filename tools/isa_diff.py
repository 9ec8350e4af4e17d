#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two `hipcc --cuda-device-only -S` outputs.

    python tools/isa_diff.py old.s new.s          # two files
    python tools/isa_diff.py old_dir new_dir      # every *.s of two directories, paired by file name
Per kernel it compares the instruction text (comments dropped, the function number taken out of the block labels) and the
VGPR / AGPR / SGPR / LDS / scratch sizes of the code object's metadata, and prints three lists: identical, changed, present
on one side only.  A one-sided kernel whose text and sizes equal a one-sided kernel of the other side is shown as renamed.
Exit status 1 if a kernel changed.
"""
import os
import re
import subprocess
import sys

SIZES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{mangled name: (instruction lines, sizes)} of one assembly file."""
    lines = open(path).read().split("\n")
    meta = lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]
    sizes = {}
    for entry in "\n".join(meta).split("\n  - ")[1:]:            # one list item per kernel; its own keys sit at indent 4
        keys = dict(re.findall(r"^\.(\w+):[ ]+(\S+)$", re.sub(r"^    (?=\.)", "", entry, flags=re.M), flags=re.M))
        if "name" in keys:                                       # (the version list that follows has items too)
            sizes[keys["name"]] = {k: keys.get(k) for k in SIZES}
    out = {}
    for name in sizes:
        s = lines.index(next(l for l in lines if l.startswith(name + ":")))
        e = next(i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body, skip = [], False
        for l in lines[s + 1:e]:
            t = l.split(";")[0].strip()
            if t.startswith(".amdhsa_kernel"):
                skip = True
            if not skip and t and not t.startswith((".section", ".p2align")):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
            if t.startswith(".end_amdhsa_kernel"):
                skip = False
        out[name] = (body, sizes[name])
    return out


def load(path):
    if os.path.isdir(path):
        files = sorted(f for f in os.listdir(path) if f.endswith(".s"))
        return {(f, k): v for f in files for k, v in kernels(os.path.join(path, f)).items()}
    return {("", k): v for k, v in kernels(path).items()}


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, res))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = load(sys.argv[1]), load(sys.argv[2])
    pretty = demangle(sorted({k[1] for k in list(old) + list(new)}))
    show = lambda k: (k[0] + ": " if k[0] else "") + pretty[k[1]]
    both = sorted(set(old) & set(new))
    same = [k for k in both if old[k] == new[k]]
    changed = [k for k in both if old[k] != new[k]]
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    renamed = []
    for k in list(only_old):
        twin = next((n for n in only_new if new[n] == old[k]), None)
        if twin:
            renamed.append((k, twin))
            only_old.remove(k)
            only_new.remove(twin)
    print("old: %s (%d kernels)\nnew: %s (%d kernels)" % (sys.argv[1], len(old), sys.argv[2], len(new)))
    print("\nidentical (%d): same instruction text, same register / LDS / scratch sizes" % len(same))
    for k in same:
        print("  " + show(k))
    print("\nchanged (%d)" % len(changed))
    for k in changed:
        what = [s for s in SIZES if old[k][1].get(s) != new[k][1].get(s)]
        print("  %s  [%s]" % (show(k), ", ".join(["%s %s -> %s" % (s, old[k][1].get(s), new[k][1].get(s)) for s in what] +
                                                 (["text: %d -> %d lines" % (len(old[k][0]), len(new[k][0]))] if old[k][0] != new[k][0] else []))))
    print("\nrenamed, otherwise identical (%d)" % len(renamed))
    for k, n in renamed:
        print("  %s  ->  %s" % (show(k), show(n)))
    print("\nonly in old (%d)" % len(only_old))
    for k in only_old:
        print("  " + show(k))
    print("\nonly in new (%d)" % len(only_new))
    for k in only_new:
        print("  " + show(k))
    sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
