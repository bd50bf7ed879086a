#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of device assembly files, kernel by kernel.

    hipcc <build.FLAGS> --cuda-device-only -S unit.hip -o unit.s        (once per unit, on each side)
    python scripts/kernel_asm_diff.py old.s [old2.s ...] -- new.s [new2.s ...]

For a change that only moves code between translation units (profiles/volume_split.md).  Per kernel symbol it compares the
instruction stream (symbol label to its .Lfunc_end) and the .amdhsa_kernel block.  .file / .loc / .ident / .cfi lines and comments
(whole lines and trailing ones) are dropped, and the compiler's file-local label numbers (.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>,
.LJTI<n>_) are renumbered per kernel in order of appearance, since they count functions and labels of the whole file.  Exit
status 0: same kernel symbols, every stream and every block identical.
"""
import re
import sys

DROP = re.compile(r"^\s*(\.file|\.loc|\.ident|\.cfi_\w+)\b|^\s*;")
LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI)(\d+)")


def normalise(lines):
    seen = {}

    def sub(m):
        key = (m.group(1), m.group(2))
        return ".%s#%d" % (m.group(1), seen.setdefault(key, len([k for k in seen if k[0] == m.group(1)])))

    return [LABEL.sub(sub, ln.split(";")[0].rstrip()) for ln in lines if ln.strip() and not DROP.match(ln)]   # (trailing comments name basic blocks by file-local number too)


def kernels(paths):
    """{symbol: (instruction stream, .amdhsa_kernel block)} over the files."""
    out = {}
    for path in paths:
        lines = open(path).read().splitlines()
        names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            d0 = next(i for i, ln in enumerate(lines) if ln.strip() == ".amdhsa_kernel " + name)
            d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            assert name not in out, "kernel %s defined twice" % name
            out[name] = (normalise(lines[start:end]), normalise(lines[d0:d1 + 1]))
    return out


def main(argv):
    cut = argv.index("--")
    old, new = kernels(argv[:cut]), kernels(argv[cut + 1:])
    bad = 0
    for name in sorted(set(old) ^ set(new)):
        print("only in %s: %s" % ("old" if name in old else "new", name))
        bad += 1
    for name in sorted(set(old) & set(new)):
        for what, a, b in (("instructions", old[name][0], new[name][0]), ("descriptor", old[name][1], new[name][1])):
            if a != b:
                first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print("%s differ in %s at line %d of %d / %d" % (what, name, first, len(a), len(b)))
                for side in (a, b):
                    print("    " + (side[first] if first < len(side) else "<end>"))
                bad += 1
    insts = sum(len(v[0]) for v in new.values())
    print("kernels: %d old, %d new; %d lines of instruction stream compared; %d differences" % (len(old), len(new), insts, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
