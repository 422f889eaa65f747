#!/usr/bin/env python3
"""The node step of Trav::round's descent loop in two disassemblies of rt_kernels.hip: equal vector and LDS work?

    tools/descent_step_check.py parent.s tree.s [kernel-regex [kernel-regex of the second file]]
    tools/descent_step_check.py tree.s tree.s k_render_persistILb0ELi262530E k_render_persistILb0ELi386E

(the second form: the tree's own twin with the compiler's loop against the instance with the hand-written one, from one
disassembly, so that an edit of the step in round() that the assembly block does not mirror shows without the parent)

A step is the text from a pair of adjacent ds_read_b128 (the node's two halves) to the v_lshl_add_u32 behind the next
ds_write_b32 (the stack pointer's update).  For every step of the kernel (default: k_render_persist<false, 386>, mangled)
the tool prints its instruction counts and compares the multisets of v_* and ds_* mnemonics, step by step in file order
(compares ignore the _e32 / _e64 encoding suffix).  Exit status 1 if a pair differs or the numbers of steps do.  It
looks at nothing else: registers, waits, scalar and branch instructions are free to differ.
"""
import collections
import re
import sys


def kernel_text(asm, pattern):
    lines = asm.splitlines()
    rx = re.compile(pattern)
    for i, line in enumerate(lines):
        if not line.startswith((".", "\t", " ", ";")) and line.split(":")[0] and rx.search(line.split(":")[0]):
            j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
            return lines[i + 1:j]
    raise SystemExit("no kernel matches %s" % pattern)


def mnemonics(lines):
    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if line and not line.endswith(":") and not line.startswith("."):
            out.append(line.split()[0])
    return out


def steps(ms):
    out, i = [], 0
    while i + 1 < len(ms):
        if ms[i] == ms[i + 1] == "ds_read_b128":
            w = ms.index("ds_write_b32", i)
            e = ms.index("v_lshl_add_u32", w)
            out.append(ms[i:e + 1])
            i = e
        i += 1
    return out


def work(step):
    return collections.Counter(re.sub(r"_e(32|64)$", "", m) for m in step if m.startswith(("v_", "ds_")))


def main():
    pattern = sys.argv[3] if len(sys.argv) > 3 else r"k_render_persistILb0ELi386E"
    patterns = (pattern, sys.argv[4] if len(sys.argv) > 4 else pattern)
    a, b = (steps(mnemonics(kernel_text(open(p).read(), rx))) for p, rx in zip(sys.argv[1:3], patterns))
    bad = len(a) != len(b)
    print("%d steps, %d steps" % (len(a), len(b)))
    for n, (x, y) in enumerate(zip(a, b)):
        wx, wy = work(x), work(y)
        print("step %d: %d vector + %d LDS of %d | %d vector + %d LDS of %d: %s" % (
            n, sum(v for k, v in wx.items() if k[0] == "v"), sum(v for k, v in wx.items() if k[0] == "d"), len(x),
            sum(v for k, v in wy.items() if k[0] == "v"), sum(v for k, v in wy.items() if k[0] == "d"), len(y),
            "equal" if wx == wy else "DIFFERENT %s" % dict((wx - wy) + (wy - wx))))
        bad |= wx != wy
    return int(bad)


if __name__ == "__main__":
    sys.exit(main())
