#!/usr/bin/env python3
"""One line per kernel instance of a source under csrc/: name, instruction count, SHA-1 of its instructions.

    tools/kernel_digest.py [rt_kernels.hip] > digest.txt
    tools/kernel_digest.py --compare digest_parent.txt digest.txt [--map names.map]

The first form compiles the source for the device only, with the Makefile's flags, into a temporary directory (no GPU)
and digests every kernel's assembly (and that of the few device functions that are called, not inlined): two builds of
a kernel have the same digest exactly when they have the same instructions and the same block structure.  What is hashed is the kernel's text from its label to its end marker
without comments, blank lines and assembler directives, with every mangled symbol replaced by one token and the block
labels' function number dropped (.LBB12_3 -> .LBB_3), so a kernel's name and its position in the file do not count.

--compare reads two such listings and reports every kernel whose digest differs or that only one side has; it exits 1
if there is any.  --map names a file of `old => new` lines for instances that were renamed between A and B: `old` is a
regular expression matched against the whole name in A, `new` its replacement (\\1 ... for groups); `#` starts a comment.
Digests are all that is compared: the tool knows nothing about particular instructions.
"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-engine_amd")

_SYMBOL = re.compile(r"\b_Z\w+")
_BLOCK = re.compile(r"\.LBB\d+_")
_LABEL = re.compile(r"^[.\w$]+:$")


def normalise(text):
    """The lines of a kernel's text that count: instructions and block labels, names and numbering taken out."""
    out = []
    for line in text.splitlines():
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith(".") and not _LABEL.match(line):
            continue  # an assembler directive
        out.append(_BLOCK.sub(".LBB_", _SYMBOL.sub("SYM", " ".join(line.split()))))
    return out


def kernels(asm):
    """{mangled name: text from the label to its .Lfunc_end} for every function of an assembly file, in file order: the
    kernels, and the device functions that were not inlined into them (their callers' digests do not cover them)."""
    lines = asm.splitlines()
    start = {}
    for i, line in enumerate(lines):
        m = re.match(r"^([\w$.]+):", line)
        if m and not line.startswith(".L"):
            start.setdefault(m.group(1), i)
    out = {}
    for name in re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M):
        i = start[name]
        j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
        out[name] = "\n".join(lines[i + 1:j])
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not names or not os.path.exists(tool):
        return list(names)
    return subprocess.run([tool] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()


def short_name(name):
    """`void rtk::k<1, 2>(rtk::DevScene, ...)` -> `k<1, 2>`: the parameter list, the return type and the namespace go."""
    name = name.replace("(anonymous namespace)::", "")
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                name = name[:i]
                break
    return re.sub(r"^void (rtk::)?", "", name)


def listing(asm, demangler=demangle):
    """[(name, instruction count, digest)] of an assembly file's kernels, sorted by name."""
    ks = kernels(asm)
    rows = []
    for name, text in zip(demangler(list(ks)), ks.values()):
        body = normalise(text)
        count = sum(1 for l in body if not _LABEL.match(l))
        rows.append((short_name(name), count, hashlib.sha1("\n".join(body).encode()).hexdigest()))
    return sorted(rows)


def read_listing(path):
    rows = []
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                name, count, sha = line.rstrip("\n").rsplit(None, 2)
                rows.append((name, int(count), sha))
    return rows


def read_map(path):
    rules = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if line:
                old, new = line.split("=>")
                rules.append((old.strip(), new.strip()))
    return rules


def rename(name, rules):
    for old, new in rules:
        m = re.fullmatch(old, name)
        if m:
            return m.expand(new)
    return name


def compare(a, b, rules=()):
    """The differences between listings a and b, a's names taken through the rules: [(name in b, what differs)]."""
    A = {rename(n, rules): (c, s) for n, c, s in a}
    B = {n: (c, s) for n, c, s in b}
    diffs = []
    for n in sorted(set(A) | set(B)):
        if n not in B:
            diffs.append((n, "only in the first"))
        elif n not in A:
            diffs.append((n, "only in the second"))
        elif A[n][1] != B[n][1]:
            diffs.append((n, "%d instructions %s -> %d instructions %s" % (A[n] + B[n])))
    return diffs


def hipflags():
    """HIPFLAGS of the package's Makefile, with its include paths"""
    mk = open(os.path.join(PKG, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(PKG, "host")]
    return [f for f in flags if f != "$(INC)"] + inc


def compile_asm(source):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        subprocess.run([hipcc] + hipflags() + ["--cuda-device-only", "-S", "-o", out, os.path.join(PKG, "csrc", source)], check=True)
        with open(out) as f:
            return f.read()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("source", nargs="?", default="rt_kernels.hip", help="a file under csrc/")
    ap.add_argument("--asm", metavar="FILE", help="digest this assembly file instead of compiling the source")
    ap.add_argument("--compare",nargs=2, metavar=("A", "B"), help="two listings to compare instead of compiling")
    ap.add_argument("--map", help="renamed instances: lines of `old regex => new name`")
    args = ap.parse_args()
    if args.compare:
        a, b = (read_listing(p) for p in args.compare)
        diffs = compare(a, b, read_map(args.map) if args.map else ())
        for name, what in diffs:
            print("%s: %s" % (name, what))
        print("%d kernels, %d kernels: %d differences" % (len(a), len(b), len(diffs)))
        return 1 if diffs else 0
    for name, count, sha in listing(open(args.asm).read() if args.asm else compile_asm(args.source)):
        print("%-96s %6d %s" % (name, count, sha))
    return 0


if __name__ == "__main__":
    sys.exit(main())
