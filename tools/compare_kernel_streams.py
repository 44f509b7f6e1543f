#!/usr/bin/env python3
"""Compare the instruction streams of the kernels of two builds of one HIP source file.

    hipcc <the Makefile's flags> -save-temps -c lg_bundle.hip     (once per commit, each in a directory of its own)
    tools/compare_kernel_streams.py OLD.s NEW.s [--drop-trailing-false]

Reads the two gfx950 assembly files, takes every kernel's body (from its label to its .Lfunc_end), drops comments and directives, numbers the local labels
by kernel, and prints one line per kernel of OLD: identical / DIFFERENT / missing in NEW, plus the kernels NEW adds.  A kernel that gained a trailing
`false` template argument in NEW (`ba_cost_kernel<0>` -> `ba_cost_kernel<0, false>`) is matched to its old name with --drop-trailing-false.  Exit status 1
if a kernel of OLD differs or is missing.  No GPU."""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{demangled name: [instruction lines]} of every .amdhsa kernel in the file"""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        body = []
        for line in m.group(1).splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                if re.match(r"\.LBB\d+_\d+:", line):
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line).replace(name, "<self>"))
        out[name] = body
    plain = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True, check=True).stdout.split("\n")
    # the key is the kernel's name with its template arguments; the return type and the parameter list are dropped (a kernel has no overloads here)
    return {re.sub(r"^void ", "", plain[i]).split("(")[0]: body for i, body in enumerate(out.values())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop-trailing-false", action="store_true")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    if args.drop_trailing_false:
        renamed = {}
        for name, body in new.items():
            short = re.sub(r", false>$", ">", name) if name.endswith(", false>") else re.sub(r"<false>$", "", name)
            renamed[short if short in old and name not in old else name] = body
        new = renamed
    bad = 0
    for name, body in old.items():
        if name not in new:
            print(f"missing in NEW   {name}")
            bad += 1
        elif body == new[name]:
            print(f"identical        {len(body):6d} lines  {name}")
        else:
            print(f"DIFFERENT        {len(body):6d} / {len(new[name]):6d} lines  {name}")
            bad += 1
    for name in new:
        if name not in old:
            print(f"new              {len(new[name]):6d} lines  {name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
