#!/usr/bin/env python3
"""Instruction streams of the kernels in two build directories, kernel by kernel (no GPU): for each named translation unit the gfx950 code
object is taken out of `NAME.hip.o` (llvm-objcopy, the offload bundler), disassembled (llvm-objdump -d) and split per kernel symbol;
addresses and encodings are stripped, and the two streams of every kernel are compared line by line.

    python tools/compare_kernel_streams.py PARENT_BUILD CHANGE_BUILD plan_gen tick_plan unicycle [--out FILE.json]

Prints - and writes to --out - per `file:kernel` "identical" or the number of differing lines (a kernel only one side has: "missing").
Exit status 0 when every kernel is identical."""
import argparse
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("WCQP_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def streams(obj, tmp):
    """{kernel: [instruction lines]} of the gfx950 code object inside `obj`"""
    fat, dev = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "unused.o")], check=True)
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + dev], check=True)
    asm = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", dev], check=True, capture_output=True, text=True).stdout
    syms = subprocess.run([LLVM + "/llvm-readelf", "-sW", dev], check=True, capture_output=True, text=True).stdout
    kernels = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.strip().endswith(".kd")}
    out, cur = {}, None
    for ln in asm.splitlines():
        m = re.match(r"^[0-9a-f]* ?<([^>]+)>:\s*$", ln)
        if m:                                       # (a symbol: a kernel, or a function a kernel calls - compared like one)
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip():
            # (an instruction with its operands; what follows "//" is the address and the encoding)
            cur.append(re.sub(r"\s+", " ", ln.split("//")[0]).strip())
    assert kernels <= set(out), sorted(kernels - set(out))
    return out


def demangle(names):
    """{symbol: kernel name with its template arguments, without namespace or parameter list}"""
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, r):
        depth, keep = 0, []
        for ch in re.sub(r"\(anonymous namespace\)::", "", d):
            if ch == "(" and depth == 0:
                break
            depth += (ch == "<") - (ch == ">")
            keep.append(ch)
        out[n] = re.sub(r"^void ", "", "".join(keep)).strip()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("units", nargs="+")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for unit in a.units:
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            sa = streams(os.path.join(a.parent, unit + ".hip.o"), ta)
            sb = streams(os.path.join(a.change, unit + ".hip.o"), tb)
        names = demangle(sorted(set(sa) | set(sb)))
        for k in sorted(names):
            key = "%s.hip:%s" % (unit, names[k])
            if k not in sa or k not in sb:
                res[key] = {"result": "missing", "in": "parent" if k in sa else "change"}
                continue
            n = sum(1 for d in difflib.ndiff(sa[k], sb[k]) if d[:1] in "+-") if sa[k] != sb[k] else 0
            res[key] = {"result": "identical", "instructions": len(sa[k])} if n == 0 else {"result": "differs", "differing_lines": n,
                                                                                            "instructions": [len(sa[k]), len(sb[k])]}
    for k, v in res.items():
        print(k, json.dumps(v))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(0 if all(v["result"] == "identical" for v in res.values()) else 1)


if __name__ == "__main__":
    main()
