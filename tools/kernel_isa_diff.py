#!/usr/bin/env python3
"""Compare two device assembly files function by function: does a source change leave the emitted code of the kernels as it was?

    hipcc <the library's HIPCC_FLAGS without -shared -fPIC> --cuda-device-only -S csrc/mvn_hip.hip -o tree.s     (same for the parent)
    python tools/kernel_isa_diff.py parent.s tree.s [--only REGEX]

A function runs from its `_Z...:` label to `.Lfunc_end`.  Comments and assembler directives are dropped and local labels (`.LBB...`,
`.Ltmp...`) become one token, what is left is compared as text, line by line.  Prints every function that differs or exists on one
side only with both line counts, then `same N diff M`; the `__hip_cuid_*` label (a hash of the translation unit) is no function and
never compared.  Exit status 1 if a function differs (with --only: one whose mangled or demangled name matches), else 0.
"""
import argparse
import re
import subprocess
import sys

FUNC_LABEL = re.compile(r"^(_Z[\w$.]*):")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]+[\w$.]*")


def functions(path):
    """{mangled name: [normalised instruction lines]} of one assembly file"""
    out, name, body = {}, None, None
    with open(path, errors="replace") as f:
        for raw in f:
            m = FUNC_LABEL.match(raw)
            if m:  # (a `_Z` label that no .Lfunc_end closes is a data object: dropped when the next one opens)
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if raw.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            line = raw.split(";", 1)[0].split("//", 1)[0].strip()
            if not line:
                continue
            if line.endswith(":"):  # a label inside the function
                body.append(LOCAL_LABEL.sub(".L", line))
            elif not line.startswith("."):  # (a directive otherwise)
                body.append(" ".join(LOCAL_LABEL.sub(".L", line).split()))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
        pretty = res.stdout.split("\n")[: len(names)]
        if len(pretty) == len(names):
            return dict(zip(names, pretty))
    except (OSError, subprocess.CalledProcessError):
        pass
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--only", metavar="REGEX", help="only functions whose name matches decide the exit status")
    args = ap.parse_args()
    fa, fb = functions(args.a), functions(args.b)
    names = sorted(set(fa) | set(fb))
    pretty = demangle(names)
    only = re.compile(args.only) if args.only else None
    same = diff = failed = 0
    for n in names:
        a, b = fa.get(n), fb.get(n)
        if a == b:
            same += 1
            continue
        diff += 1
        if only is None or only.search(pretty[n]) or only.search(n):
            failed += 1
        if a is None or b is None:
            print(f"only in {args.a if b is None else args.b}: {pretty[n]}  ({len(a or b)} lines)")
        else:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"differs: {pretty[n]}  ({len(a)} / {len(b)} lines, first at {first})")
    print(f"same {same} diff {diff}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
