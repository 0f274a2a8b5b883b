"""Compare the kernels of two gfx950 assembly listings of the library, kernel by kernel.

    hipcc <build.py's HIPCC_FLAGS without -shared / -ldl> --cuda-device-only -S tal_agg.hip -o X.s
    python tools/kernel_asm_diff.py parent.s new.s [--show SUBSTRING ...] [--lists DIR]
                                    [--rename REGEX REPLACEMENT ...]

A kernel is everything from its "Begin function" line to the end of its "Kernel info" block:
instructions, labels, the .amdhsa_ descriptor and the .set resource symbols.  Two kernels of
one symbol name are identical when those lines agree once comments are dropped and the number
of the function is taken out of the compiler's labels (.LBB<f>_<k>, .Lfunc_end<f>: <f> counts
the functions before it in the file).  The resource lines of the "Kernel info" comments (SGPRs,
VGPRs, AGPRs, scratch, LDS, occupancy) are compared separately.  Prints the kernels only one
side has, the count of identical ones, a unified diff of each that differs, and the resources
of the kernels whose name contains a --show substring; --lists writes kernels_parent.txt and
kernels_new.txt (one symbol per line) into DIR.  --rename rewrites the parent's symbols (in the
kernels' names and wherever their lines spell them) before the comparison: a kernel whose
template or argument list grew is then held against the instantiation that took its place, and
what still differs (the kernarg size, say) is printed.  Exit status 1 when a common kernel differs.
"""
from __future__ import annotations

import argparse
import difflib
import re
import sys
from pathlib import Path

_BEGIN = re.compile(r"; -- Begin function (\S+)")
_LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")
_RES = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path: Path, renames=()) -> dict:
    """{symbol: (normalized lines, {resource: value})} of every kernel in the listing."""
    out, name, lines, res, in_info = {}, None, [], {}, False
    text = path.read_text()
    for pat, repl in renames:
        text = re.sub(pat, repl, text)

    def close():
        if name is not None and any(ln.startswith(".amdhsa_kernel ") for ln in lines):
            out[name] = (lines, res)

    for raw in text.splitlines():
        m = _BEGIN.search(raw)
        if m:
            close()
            name, lines, res, in_info = m.group(1), [], {}, False
        if name is None:
            continue
        if in_info and not raw.startswith(";"):
            close()
            name = None
            continue
        if raw.startswith("; Kernel info:"):
            in_info = True
        if in_info:
            key, _, val = raw[2:].partition(":")
            if key.strip() in _RES:
                res[key.strip()] = val.strip()
            continue
        code = _LABEL.sub(r".\1", raw.split(";", 1)[0]).strip()
        if code:
            lines.append(code)
    close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--show", action="append", default=[], help="print the resources of kernels whose name contains this")
    ap.add_argument("--lists", type=Path, help="directory for kernels_parent.txt / kernels_new.txt")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPLACEMENT"),
                    help="rewrite the parent's symbols before comparing")
    args = ap.parse_args()
    a, b = kernels(args.parent, args.rename), kernels(args.new)
    if args.lists:
        (args.lists / "kernels_parent.txt").write_text("".join(k + "\n" for k in a))
        (args.lists / "kernels_new.txt").write_text("".join(k + "\n" for k in b))
    print(f"kernels: parent {len(a)}, new {len(b)}")
    for tag, only in (("parent", [k for k in a if k not in b]), ("new", [k for k in b if k not in a])):
        print(f"only in {tag}: {len(only)}")
        for k in only:
            print(f"   {k}")
    common = [k for k in a if k in b]
    differ = [k for k in common if a[k] != b[k]]
    print(f"common kernels: {len(common)}; instructions, descriptor and resources identical: "
          f"{len(common) - len(differ)} of {len(common)}")
    for k in differ:
        print(f"== {k}\n   resources parent {a[k][1]}\n   resources new    {b[k][1]}")
        for ln in difflib.unified_diff(a[k][0], b[k][0], "parent", "new", n=1, lineterm=""):
            print("   " + ln)
    for sub in args.show:
        for side, ks in (("parent", a), ("new", b)):
            for k in ks:
                if sub in k:
                    print(f"{side:6s} {k}: {len(ks[k][0])} lines; " + " ".join(f"{r}={v}" for r, v in ks[k][1].items()))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
