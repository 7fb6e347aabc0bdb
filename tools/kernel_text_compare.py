#!/usr/bin/env python3
"""Compare two device-only assembly listings kernel by kernel: tools/kernel_text_compare.py A.s B.s [--require NAME ...] [--label TEXT]

The listings come from `hipcc <the library's flags> --cuda-device-only -S -o X.s mpc_amd.hip`.  Per kernel symbol (`.amdhsa_kernel`) the
instruction stream is compared with comments, directives and blank lines dropped and the function number taken out of the block labels
(`.LBB12_34` -> `.LBB_34`) and the module-wide counter out of the labels of long branches (`.Lpost_getpc31`): one line `SAME` / `DIFF`, the instruction counts and the private-segment sizes of both sides, the demangled
name.  Exit status 1 if a kernel is in one listing only, or if a kernel whose name starts with one of the --require names (followed by
`<`, or by `(` for a kernel that is no template) is not SAME."""
import argparse
import re
import shutil
import subprocess
import sys


def kernels(path):
    """{symbol: (instruction lines, private segment bytes)} of the kernels of one listing"""
    bodies, cur, buf, priv, names = {}, None, [], {}, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if cur is None and m and not m.group(1).startswith(".L"):
            cur, buf = m.group(1), []
            continue
        if cur is not None and line.startswith(".Lfunc_end"):
            bodies[cur], cur = buf, None
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            names.append(m.group(1))
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m and names:
            priv[names[-1]] = int(m.group(1))
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        buf.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", s)))
    return {k: (bodies[k], priv.get(k, -1)) for k in names if k in bodies}


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool or not symbols:
        return {s: s for s in symbols}
    out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True).stdout.split("\n")
    return {s: re.sub(r"^void |\(mpc::DevProblem const\*.*$", "", d) for s, d in zip(symbols, out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--require", nargs="*", default=[], help="kernel templates every instantiation of which has to be SAME")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    ka, kb = kernels(args.a), kernels(args.b)
    names = demangle(sorted(set(ka) | set(kb)))
    print(f"# {args.label or args.a + ' vs ' + args.b}: {len(ka)} | {len(kb)} kernels; verdict, instructions a | b, private segment bytes a | b, kernel")
    ok = True
    for sym in sorted(names, key=names.get):
        if sym not in ka or sym not in kb:
            print(f"ONLY-{'A' if sym in ka else 'B'}  {names[sym]}")
            ok = False
            continue
        (ta, pa), (tb, pb) = ka[sym], kb[sym]
        same = ta == tb
        print(f"{'SAME' if same else 'DIFF'}  {len(ta):6d} | {len(tb):6d}  {pa:6d} | {pb:6d}  {names[sym]}")
        if not same and any(names[sym].startswith((r + "<", r + "(")) for r in args.require):
            print(f"      ^ required to be SAME")
            ok = False
    print("REQUIRED KERNELS SAME" if ok else "FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
