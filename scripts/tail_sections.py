"""Static instruction counts of the Gauss-Newton tail (kt_solve_and_update_wave) by section, and the register budget of the four
kernels that end in it.  Compiles csrc/kt_track.hip to gfx950 assembly with -DKT_TAIL_MARK (device only, no GPU needed) and counts the
instructions that follow each "; TAILSEC n" marker up to the next one, in text order: both sides of every branch are included.
    python scripts/tail_sections.py [kernel substring, default kt_icp_level_kernel] [--csrc DIR]
--csrc DIR reads another checkout's kintinuous_amd/csrc (the parent commit's, for a before / after table)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kintinuous_amd import build  # noqa: E402

KERNELS = ("kt_icp_level_kernel", "kt_icp_kernel", "kt_rgb_kernel", "kt_joint_kernel")
GROUPS = (("1", ("1",)), ("2 / 3 / 31", ("2", "3", "31")), ("4", ("4",)), ("5 / 6 / 7", ("5", "6", "7")), ("8", ("8",)), ("9 / 10 / 11", ("9", "10")))
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")


def assembly(csrc, marks):
    out = os.path.join(tempfile.mkdtemp(), "kt_track.s")
    subprocess.check_call([build.hipcc()] + build.FLAGS + (["-DKT_TAIL_MARK"] if marks else []) + ["-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                                                                     "-o", out, os.path.join(csrc, "kt_track.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_body(text, sub):
    for m in re.finditer(r"^(_Z\w*" + re.escape(sub) + r"\w*):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        return m.group(1), m.group(0)
    raise SystemExit("no kernel matches " + sub)


def main():
    args = sys.argv[1:]
    csrc = build.CSRC
    if "--csrc" in args:
        k = args.index("--csrc")
        csrc = args[k + 1]
        del args[k:k + 2]
    sub = args[0] if args else "kt_icp_level_kernel"
    name, body = kernel_body(assembly(csrc, True), sub)
    counts, kinds = collections.Counter(), collections.defaultdict(collections.Counter)
    sec, total = None, 0
    for line in body.splitlines():
        m = re.search(r"; TAILSEC (\d+)", line)
        if m:
            sec = m.group(1)
            continue
        m = INSN.match(line)
        if not m or line.lstrip().startswith((".", ";")):
            continue
        total += 1
        if sec is not None and sec != "11":
            counts[sec] += 1
            op = m.group(1)
            kinds[sec]["SALU" if op.startswith("s_") and not op.startswith("s_nop") else "s_nop" if op.startswith("s_nop") else "readlane" if "readlane" in op
                       else "f64" if op.endswith("_f64") else "LDS" if op.startswith("ds_") else "other VALU" if op.startswith("v_") else "memory"] += 1
    print("# %s: %d instructions, %d of them in the tail\n" % (sub, total, sum(counts.values())))
    print("| section | instructions | SALU | s_nop | readlane | f64 | LDS | other VALU | memory |")
    print("|---|---|---|---|---|---|---|---|---|")
    for label, secs in GROUPS:
        kk = collections.Counter()
        for s in secs:
            kk.update(kinds[s])
        print("| %s | %d | %s |" % (label, sum(counts[s] for s in secs), " | ".join(str(kk[c]) for c in ("SALU", "s_nop", "readlane", "f64", "LDS", "other VALU", "memory"))))
    plain = assembly(csrc, False)
    meta = plain[plain.index("amdhsa.kernels:"):]
    print("\n| kernel | VGPR | VGPR spills | scratch bytes |")
    print("|---|---|---|---|")
    for blk in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: (re.search(r"\." + key + r":\s+(\S+)", blk) or [None, "?"])[1]
        for kn in KERNELS:
            if re.search(r"\d" + kn + r"[A-Z0-9]", get("name")):
                print("| %s | %s | %s | %s |" % (kn, get("vgpr_count"), get("vgpr_spill_count"), get("private_segment_fixed_size")))


if __name__ == "__main__":
    main()
