#!/usr/bin/env python3
"""Are the kernels of two hipcc -S listings the same instruction for instruction?  Every kernel whose mangled name matches the
pattern is cut out of both listings as tools/isa_extract.py cuts it (label to s_endpgm) and compared once the function's number
in its local labels (.LBB<n>_k, also where comments name them) is taken out.
   python tools/isa_compare.py before.s after.s 'k_deform32_|k_vectors32_shared_'
Listings: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I include <the file's extra flags of
facedeform_amd/_build.py> --cuda-device-only -S -x hip facedeform_amd/csrc/<file>.hip -o <file>.s
Exit status 1 when a body differs or the two listings do not hold the same kernels."""
import hashlib
import re
import sys


def bodies(path, pattern):
    lines = open(path).read().split("\n")
    out = {}
    for i, l in enumerate(lines):
        if re.search(pattern, l) and l.split(";")[0].strip().endswith(":") and not l.startswith((".", ";", "\t")):
            end = next(k for k in range(i, len(lines)) if lines[k].strip().startswith("s_endpgm"))
            body = "\n".join(lines[i:end + 1])
            body = re.sub(r"BB\d+_(\d+)", r"BB_\1", body)
            out[l.split(":")[0]] = re.sub(r"[ \t]+;", " ;", body)       # (the comment column behind a label moves with the number's width)
    return out


def main():
    a, b = bodies(sys.argv[1], sys.argv[3]), bodies(sys.argv[2], sys.argv[3])
    differ = sorted(set(a) ^ set(b))
    for k in differ:
        print("ONLY IN ONE", k)
    for k in sorted(set(a) & set(b)):
        same = a[k] == b[k]
        differ += [] if same else [k]
        print("%s %6d lines %s %s" % ("same" if same else "DIFF", a[k].count("\n") + 1, hashlib.sha256(b[k].encode()).hexdigest()[:12], k))
    print("%d kernels, %d differ" % (len(set(a) | set(b)), len(differ)))
    sys.exit(1 if differ or not a else 0)


if __name__ == "__main__":
    main()
