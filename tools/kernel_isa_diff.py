#!/usr/bin/env python3
r"""Compare the device code of two trees kernel by kernel (no GPU, no torch).

    python tools/kernel_isa_diff.py OLD_ROOT NEW_ROOT projection.hip surfel.hip \
        --require '*projection_bwd_kernel*' --require 'surfel.hip:*'

Each file of gsplat-triton_amd/csrc is compiled in both trees to gfx950
assembly with the flags of that tree's Makefile (CXXFLAGS, EXTRA_<file>) plus
--cuda-device-only -S.  A kernel is its text from the entry label through
.end_amdhsa_kernel, so the descriptor's register, LDS and scratch figures are
compared too, and printed for a kernel that differs (next_free_vgpr /
accum_offset / next_free_sgpr / LDS / scratch bytes).  Local labels are
compared without the function's position in its file (.LBB7_3 as .LBB_3),
which moves when a file is split, and a kernel's own symbol as <kernel>.  A
file argument OLD.hip=NEW.hip compares OLD.hip of the old tree with NEW.hip
of the new one; --rename REGEX=REPL is applied to the old tree's demangled
names first (a kernel that lost a template parameter:
--rename '(fwd2_kernel<\d+), false>=\1>').  --require takes fnmatch patterns
over "file:demangled name" (the new tree's file name); the exit status is 1 if
a kernel that matches one differs or is missing."""
import argparse, difflib, fnmatch, os, re, shutil, subprocess, sys


def flags(csrc, name):
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda v: (re.search(rf"^{re.escape(v)}\s*[:?]?=\s*(.*)$", mk, re.M) or [None, ""])[1]
    cxx = var("CXXFLAGS").replace("$(ARCH)", var("ARCH") or "gfx950")
    return cxx.split() + var("EXTRA_" + name).split()


def kernels(root, name):
    """{demangled kernel name: its assembly lines} of one file of one tree."""
    csrc = os.path.join(root, "gsplat-triton_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = subprocess.run([hipcc, *flags(csrc, name), "--cuda-device-only", "-S", name, "-o", "-"],
                         cwd=csrc, check=True, capture_output=True, text=True).stdout
    # local labels carry the function's position in its file (.LBB7_3, .Lfunc_end7),
    # which moves when a file is split: compared without it
    lines = [re.sub(r"(\.LBB|\bBB|\.Lfunc_end|\.LJTI)\d+", r"\1", l)
             for l in asm.splitlines() if "__hip_cuid" not in l]
    syms = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    filt = next(filter(None, map(shutil.which, ("llvm-cxxfilt", "c++filt", "x86_64-linux-gnu-c++filt"))), None)
    plain = subprocess.run([filt, "-p", *syms], check=True, capture_output=True,
                           text=True).stdout.split("\n") if filt else syms
    out = {}
    for sym, nice in zip(syms, plain):  # -p: names without their parameter lists
        a = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        b = lines.index("\t.end_amdhsa_kernel", a)
        out[nice] = [l.replace(sym, "<kernel>") for l in lines[a:b + 1]]
    return out


def figures(body):
    val = {l.split()[0]: l.split()[-1] for l in body if l.strip().startswith(".amdhsa_")}
    return "/".join(val.get(".amdhsa_" + f, "?") for f in (
        "next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size",
        "private_segment_fixed_size"))


def n_instr(body):
    return sum(1 for l in map(str.strip, body) if l and l[0] not in ".;" and not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("old_root")
    ap.add_argument("new_root")
    ap.add_argument("files", nargs="+",
                    help=".hip files under gsplat-triton_amd/csrc (NAME.hip or OLD.hip=NEW.hip)")
    ap.add_argument("--require", action="append", default=[], metavar="PATTERN")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    args = ap.parse_args()
    bad = 0
    for arg in args.files:
        old_name, _, name = arg.rpartition("=")  # OLD.hip=NEW.hip: a file that was renamed or split
        old, new = kernels(args.old_root, old_name or name), kernels(args.new_root, name)
        for r in args.rename:
            old = {re.sub(*r.rsplit("=", 1), k): v for k, v in old.items()}
        for k in list(old) + [k for k in new if k not in old]:
            if k not in old or k not in new:
                verdict = "only in " + (args.old_root if k in old else args.new_root)
            elif old[k] == new[k]:
                verdict = "identical"
            else:
                d = sum(1 for l in difflib.unified_diff(old[k], new[k], lineterm="", n=0)
                        if l[0] in "+-" and l[:3] not in ("+++", "---"))
                verdict = (f"{d} lines differ, instructions {n_instr(old[k])} -> {n_instr(new[k])}, "
                           f"registers {figures(old[k])} -> {figures(new[k])}")
            required = any(fnmatch.fnmatchcase(f"{name}:{k}", p) for p in args.require)
            if required and verdict != "identical":
                bad = 1
                verdict += "  <-- REQUIRED identical"
            print(f"{name:22s} {k:60s} {verdict}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
