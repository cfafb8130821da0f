#!/usr/bin/env python3
"""Compares the kernels of two device assembly files (hipcc -save-temps=obj:
<unit>-hip-amdgcn-amd-amdhsa-gfx950.s) body by body.

    isa_compare.py A.s B.s [--list]

A kernel's body is the text between its label and its .Lfunc_end, without
comments, blank lines and debug / line directives.  Prints the number of
kernels in each file, of kernels only one file has, and of common kernels
whose bodies are identical / differ; every differing or unmatched kernel by
name.  Exit status 0 only when both files hold the same kernels with
identical bodies.
"""
import argparse
import hashlib
import re
import sys

_SKIP = re.compile(r"^\s*(\.loc|\.file|\.cfi_|\.ident|\.section\s+\.debug)")


def kernels(path):
    """{kernel name: sha256 of its stripped body}"""
    out, name, body = {}, None, []
    with open(path, errors="replace") as f:
        for line in f:
            if name is None:
                m = re.match(r"^([A-Za-z_][\w$.]*):", line)
                if m and not m.group(1).startswith(".L"):
                    name, body = m.group(1), []
                continue
            if line.startswith(".Lfunc_end"):
                out[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()
                name = None
                continue
            line = line.split(";", 1)[0].rstrip()
            if not line.strip() or _SKIP.match(line):
                continue
            # local labels carry a per-file function number: .LBB<fn>_<block>
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line.strip()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--list", action="store_true", help="also print the identical kernels' names")
    args = ap.parse_args()
    ka, kb = kernels(args.a), kernels(args.b)
    only_a = sorted(set(ka) - set(kb))
    only_b = sorted(set(kb) - set(ka))
    common = sorted(set(ka) & set(kb))
    differ = [k for k in common if ka[k] != kb[k]]
    print(f"kernels: {len(ka)} in A, {len(kb)} in B; only in A {len(only_a)}, only in B {len(only_b)}")
    print(f"common {len(common)}: identical {len(common) - len(differ)}, differing {len(differ)}")
    for tag, names in (("only in A", only_a), ("only in B", only_b), ("differs", differ)):
        for k in names:
            print(f"{tag}: {k}")
    if args.list:
        for k in common:
            if ka[k] == kb[k]:
                print(f"identical: {k}")
    return 0 if not (only_a or only_b or differ) else 1


if __name__ == "__main__":
    sys.exit(main())
