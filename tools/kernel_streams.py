#!/usr/bin/env python3
"""Are the kernels of two device-assembly files the same code?  The check behind "instruction for instruction what it was"
(DESIGN.md 4.16): CPU only, it compares text and knows no instruction.

    hipcc $(CXXFLAGS) $(FLAGS_x) --cuda-device-only -S x.hip -o new.s        (the same for the other commit: old.s)
    python3 tools/kernel_streams.py old.s new.s [--map OLD_SYMBOL=NEW_SYMBOL ...] [--diff N]

Per kernel (every symbol with a `.amdhsa_kernel` block), two lists:
  instructions  the lines from the kernel's label to its descriptor, without comments, directives and blank lines; local
                labels (.L...) are numbered afresh in the order in which the kernel names them, so a renumbering compares equal
                and a branch to another place does not;
  metadata      the descriptor (.amdhsa_*), the symbol's `.set` values, the "; Kernel info:" remarks and the kernel's entry
                of the metadata note (registers, spills, LDS, scratch, kernarg size), with the symbol's name replaced by `@`.
Kernels are paired by symbol, or by --map where the symbol changed.  One line per pair: the two instruction counts and EQUAL
or DIFF for each list; --diff N adds the first N differing lines of each list.  Exit status 1 if a pair differs or a kernel of
either file has no partner."""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L\w+")


def kernels(path):
    """{symbol: (instructions, metadata)} of one assembly file"""
    lines = open(path).read().splitlines()
    out = {}
    for name in [l.split()[1] for l in lines if l.split()[:1] == [".amdhsa_kernel"]]:
        beg = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i, l in enumerate(lines) if l.split() == [".amdhsa_kernel", name])
        labels, insts = {}, []
        for l in lines[beg + 1:end]:
            l = " ".join(l.split(";")[0].split())
            if l and (not l.startswith(".") or l.endswith(":")):
                insts.append(LOCAL.sub(lambda m: labels.setdefault(m.group(), ".L%d" % len(labels)), l))
        k = next(i for i in range(end, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        meta = lines[end:k] + [l for l in lines if l.strip().startswith(".set " + name + ".")]
        info = next((i for i in range(k, len(lines)) if lines[i].startswith("; Kernel info:")), None)
        nxt = next((i for i in range(k, len(lines)) if lines[i].split()[:1] == [".amdhsa_kernel"]), len(lines))
        if info is not None and info < nxt:     # the compiler's remarks behind this descriptor
            for l in lines[info + 1:]:
                if not l.startswith(";"):
                    break
                meta.append(l)
        note = next((i for i, l in enumerate(lines) if l.split() == [".name:", name]), None)
        if note is not None:                    # this kernel's item of the list `amdhsa.kernels:`
            lo = max(i for i in range(note + 1) if lines[i].startswith("  - "))
            hi = next((i for i in range(note + 1, len(lines)) if not lines[i].startswith("    ")), len(lines))
            meta += lines[lo:hi]
        out[name] = (insts, [" ".join(l.replace(name, "@").split()) for l in meta])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="pair a renamed kernel")
    ap.add_argument("--diff", type=int, default=0, metavar="N", help="print the first N differing lines of a DIFF")
    args = ap.parse_args(argv)
    old, new = kernels(args.old), kernels(args.new)
    renamed = dict(m.split("=", 1) for m in args.map)
    bad = 0
    for name, (oi, om) in old.items():
        to = renamed.get(name, name)
        if to not in new:
            print(f"{name}: UNPAIRED (not in {args.new})")
            bad = 1
            continue
        ni, nm = new.pop(to)
        count = lambda insts: sum(not l.endswith(":") for l in insts)
        print(f"{name}{'' if to == name else ' -> ' + to}: instructions {count(oi)} / {count(ni)} {'EQUAL' if oi == ni else 'DIFF'},"
              f" metadata {'EQUAL' if om == nm else 'DIFF'}")
        bad |= oi != ni or om != nm
        for what, a, b in (("instructions", oi, ni), ("metadata", om, nm)):
            rows = [i for i in range(max(len(a), len(b))) if a[i:i + 1] != b[i:i + 1]][:args.diff]
            for i in rows:
                print(f"    {what} [{i}]  old: {(a[i:i + 1] or ['(none)'])[0]}\n    {' ' * len(what)} {' ' * len(str(i))}   new: {(b[i:i + 1] or ['(none)'])[0]}")
    for name in new:
        print(f"{name}: UNPAIRED (not in {args.old})")
        bad = 1
    return int(bad)


if __name__ == "__main__":
    sys.exit(main())
