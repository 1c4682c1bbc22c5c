#!/usr/bin/env python3
"""Compare the device code of two trees kernel by kernel (no GPU, no torch).

    python tools/kernel_isa_diff.py OLD_ROOT NEW_ROOT projection.hip surfel.hip \
        --require '*projection_bwd_kernel*' --require 'surfel.hip:*'

Each file of gsplat-triton_amd/csrc is compiled in both trees to gfx950
assembly with the flags of that tree's Makefile (CXXFLAGS, EXTRA_<file>) plus
--cuda-device-only -S.  A kernel is its text from the entry label through
.end_amdhsa_kernel, so the descriptor's register, LDS and scratch figures are
compared too.  --require takes fnmatch patterns over "file:demangled name";
the exit status is 1 if a kernel that matches one differs or is missing."""
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
    lines = [l for l in asm.splitlines() if "__hip_cuid" not in l]
    syms = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    filt = next(filter(None, map(shutil.which, ("llvm-cxxfilt", "c++filt", "x86_64-linux-gnu-c++filt"))), None)
    plain = subprocess.run([filt, "-p", *syms], check=True, capture_output=True,
                           text=True).stdout.split("\n") if filt else syms
    out = {}
    for sym, nice in zip(syms, plain):  # -p: names without their parameter lists
        a = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        b = lines.index("\t.end_amdhsa_kernel", a)
        out[nice] = lines[a:b + 1]
    return out


def n_instr(body):
    return sum(1 for l in map(str.strip, body) if l and l[0] not in ".;" and not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("old_root")
    ap.add_argument("new_root")
    ap.add_argument("files", nargs="+", help=".hip files under gsplat-triton_amd/csrc")
    ap.add_argument("--require", action="append", default=[], metavar="PATTERN")
    args = ap.parse_args()
    bad = 0
    for name in args.files:
        old, new = kernels(args.old_root, name), kernels(args.new_root, name)
        for k in list(old) + [k for k in new if k not in old]:
            if k not in old or k not in new:
                verdict = "only in " + (args.old_root if k in old else args.new_root)
            elif old[k] == new[k]:
                verdict = "identical"
            else:
                d = sum(1 for l in difflib.unified_diff(old[k], new[k], lineterm="", n=0)
                        if l[0] in "+-" and l[:3] not in ("+++", "---"))
                verdict = f"{d} lines differ, instructions {n_instr(old[k])} -> {n_instr(new[k])}"
            required = any(fnmatch.fnmatchcase(f"{name}:{k}", p) for p in args.require)
            if required and verdict != "identical":
                bad = 1
                verdict += "  <-- REQUIRED identical"
            print(f"{name:22s} {k:60s} {verdict}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
