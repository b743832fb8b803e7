#!/usr/bin/env python3
"""Are the kernels of two source trees the same code?  Compiles every csrc/*.hip of both trees to gfx950 device assembly with the
Makefile's CXXFLAGS (+ --cuda-device-only -S) and diffs it function by function.  A tree is a directory or a git revision.
  python tools/isa_diff.py HEAD~1 . --rename g_big_zero16=g_zero16 [-D UPA_ABLATE] [--files conv_big.hip ...]
Normalised away: __hip_cuid_* names, --rename'd symbols and the definition (section, linkage, size) of a renamed data symbol,
comments.  Exit status 1 if an instruction line or an .amdhsa_* descriptor line of any function differs."""
import argparse, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = "ultralytics_pro_amd/csrc"
DATA = "(data and metadata)"


def tree(arg, tmp):
    if os.path.isdir(os.path.join(arg, CSRC)): return os.path.abspath(arg)
    dst = tempfile.mkdtemp(dir=tmp)
    tar = subprocess.run(["git", "archive", arg, CSRC, "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return dst


def assemble(root, name, defines, out):
    mk = open(os.path.join(root, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, *["-D" + d for d in defines], "--cuda-device-only", "-S", name, "-o", out]
    subprocess.run(cmd, cwd=os.path.join(root, CSRC), check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def units(asm, renames):
    """{function: [normalised lines]} plus DATA: everything outside the functions"""
    for old, new in renames: asm = re.sub(r"\b%s\b" % re.escape(old), new, asm)
    asm = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", asm)
    out, cur, skip = {DATA: []}, DATA, None
    for line in asm.split("\n"):
        if '"' not in line: line = line.split(";")[0]
        line = " ".join(line.split())
        if not line: continue
        if m := re.match(r"\.type (\S+),@function", line): cur = m.group(1); out[cur] = []
        if skip is None and (m := re.match(r"\.(?:protected|type|weak|globl) (\w+)", line)) and m.group(1) in [n for _, n in renames]: skip = m.group(1)
        # a renamed data symbol may move to a section of its own: which of its neighbours then carries the switch back is layout, not code
        if renames and cur == DATA and line.startswith(".section"): continue
        if skip is None and not line.startswith(".addrsig_sym"): out[cur].append(line)
        if skip and re.match(r"\.(size|comm) %s," % skip, line): skip = None
        if re.match(r"\.size (\S+), \.Lfunc_end", line): cur = DATA
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a"); ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--files", nargs="*")
    ap.add_argument("-v", "--verbose", action="store_true", help="one line per identical function too, not only per file")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    renames = [tuple(r.split("=")) for r in args.rename]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        a, b = tree(args.a, tmp), tree(args.b, tmp)
        files = args.files or sorted(f for f in os.listdir(os.path.join(b, CSRC)) if f.endswith(".hip"))
        with ThreadPoolExecutor(args.j) as ex:
            jobs = [(f, ex.submit(assemble, a, f, args.defines, f"{tmp}/a_{f}.s"), ex.submit(assemble, b, f, args.defines, f"{tmp}/b_{f}.s")) for f in files]
            for f, ja, jb in jobs:
                ua, ub = units(ja.result(), renames), units(jb.result(), renames)
                same = 0
                for k in list(ua) + [k for k in ub if k not in ua]:
                    la, lb = ua.get(k), ub.get(k)
                    if la == lb:
                        same += 1
                        if args.verbose: print(f"{f}: {k}: identical")
                        continue
                    if la is None or lb is None: print(f"{f}: {k}: only in {'b' if la is None else 'a'}"); bad += 1; continue
                    i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
                    print(f"{f}: {k}: DIFFERS at line {i} ({len(la)} / {len(lb)} lines)\n  a: {la[i] if i < len(la) else '<end>'}\n  b: {lb[i] if i < len(lb) else '<end>'}")
                    bad += 1
                print(f"{f}: {same} of {len(set(ua) | set(ub))} units identical ({len(ub) - 1} functions)" + ("" if same == len(set(ua) | set(ub)) else "  <-- DIFFERS"))
    print("isa_diff:", "every function and descriptor identical" if not bad else f"{bad} units differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
