#!/usr/bin/env python3
"""Is the device code of csrc files the same in two source trees?  For a host-side refactor this is the speed proof: equal instructions
take equal time.

    python tools/compare_device_code.py OTHER_TREE [--out DIR] file.hip ...

compiles csrc/<file> of this tree and of OTHER_TREE (a checkout of the commit to compare with) with the Makefile's CXXFLAGS plus
--cuda-device-only -S and -Rpass-analysis=kernel-resource-usage, and compares per kernel, matched by mangled name: the set of kernels, each
kernel's text from its label to the end of its .amdhsa_kernel block, and the resource report line for line.  Two things are normalised
and nothing else: the compile-unit id hipcc derives from the file's path (__hip_cuid_<hash>, and the same hash where it is appended to
the names of internal-linkage kernels), and the source position in front of each remark, which moves with every edited line above a
kernel.  Prints one line per file; exit status 1 if any file differs.  --out DIR keeps <file>.other.txt and <file>.this.txt, the two
normalised resource reports.  It compares text for equality and looks for nothing in particular."""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def flags(tree):
    text = open(os.path.join(tree, "mesh-reconstruction_amd", "Makefile")).read()
    return shlex.split(re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950"))


def compile_one(tree, name, tmp):
    """-> ({kernel: text}, [report lines]) of csrc/<name> in `tree`"""
    out = os.path.join(tmp, name + ".s")
    r = subprocess.run([HIPCC] + flags(tree) + ["--cuda-device-only", "-S", os.path.join("csrc", name), "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                       cwd=os.path.join(tree, "mesh-reconstruction_amd"), capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    asm = open(out).read()
    cuid = re.search(r"__hip_cuid_([0-9a-f]+)", asm)
    if cuid:
        asm = asm.replace(cuid.group(1), "CUID")
    kernels = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", asm, re.M | re.S):
        k = m.group(1)
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:\n" % re.escape(k), asm, re.M | re.S)
        kernels[k] = body.group(0) + m.group(0)
    report = [line.split("remark:", 1)[1].strip() for line in r.stderr.splitlines() if "remark:" in line and "[-Rpass-analysis" in line]
    if cuid:
        report = [line.replace(cuid.group(1), "CUID") for line in report]
    return kernels, report


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--out")
    a = ap.parse_args()
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.files:
            os.makedirs(os.path.join(tmp, "other"), exist_ok=True)
            ko, ro = compile_one(os.path.abspath(a.other), name, os.path.join(tmp, "other"))
            kt, rt = compile_one(ROOT, name, tmp)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                for tag, rep in (("other", ro), ("this", rt)):
                    open(os.path.join(a.out, "%s.%s.txt" % (name, tag)), "w").write("\n".join(rep) + "\n")
            changed = sorted(k for k in set(ko) & set(kt) if ko[k] != kt[k])
            same = set(ko) == set(kt) and not changed and ro == rt
            differ += not same
            print("%-16s %3d kernels, %6d instruction lines: %s" % (name, len(kt), sum(t.count("\n") for t in kt.values()),
                  "kernel set, every kernel's text and the resource report are equal" if same else
                  "DIFFERENT: %d kernels only there, %d only here, %d with other text, report %s" % (
                      len(set(ko) - set(kt)), len(set(kt) - set(ko)), len(changed), "equal" if ro == rt else "differs")))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
