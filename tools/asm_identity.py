#!/usr/bin/env python3
"""Is the device code of two sets of sources the same, kernel by kernel?

    python tools/asm_identity.py OLD_S... -- NEW_S...

Each argument is device assembly (the Makefile's FLAGS + --cuda-device-only -S)
of one .hip file.  Per .amdhsa_kernel name the instruction text and the
.amdhsa_ descriptor block are compared, local labels normalised (their numbers
depend on a kernel's place in its file); the device functions that were not
inlined are compared the same way.  Every kernel must be in exactly one file
of its side.  Exit status 0: the same kernels, all identical.
"""
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?\b")


def kernels(path):
    """{function name: its instructions (a kernel's .amdhsa_ descriptor block with them), comments dropped,
    labels normalised}"""
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M):
        # from the entry label to the function's end label: a kernel's descriptor block lies in between
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        if not body:
            raise SystemExit(f"{path}: cannot find the body of {name}")
        lines = [ln.split(";")[0].rstrip() for ln in body.group(0).split("\n")]
        seen = {}       # labels renumbered in order of first appearance
        out[name] = LABEL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"),
                              "\n".join(ln for ln in lines if ln.strip()))
    return out


def is_kernel(text):
    return ".end_amdhsa_kernel" in text


def side(paths):
    allk, where = {}, {}
    for p in paths:
        for name, text in kernels(p).items():
            if name in allk:
                raise SystemExit(f"{name} is in {where[name]} and in {p}")
            allk[name], where[name] = text, p
    return allk, where


def main():
    if "--" not in sys.argv:
        raise SystemExit(__doc__)
    cut = sys.argv.index("--")
    (old, _), (new, where) = side(sys.argv[1:cut]), side(sys.argv[cut + 1:])
    missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    for p in sys.argv[cut + 1:]:
        print(f"{p}: {sum(1 for k, w in where.items() if w == p and is_kernel(new[k]))} kernels")
    nk = [sum(map(is_kernel, s.values())) for s in (old, new)]
    print(f"old {nk[0]} kernels (+ {len(old) - nk[0]} device functions), new {nk[1]} (+ {len(new) - nk[1]}): "
          f"{len(missing)} missing, {len(added)} added, {len(differ)} differ")
    for tag, ks in (("missing", missing), ("added", added), ("differs", differ)):
        for k in ks:
            print(f"  {tag}: {k}")
    sys.exit(1 if missing or added or differ else 0)


if __name__ == "__main__":
    main()
