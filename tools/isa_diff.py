#!/usr/bin/env python
"""Compare the gfx950 ISA of the default-format k_idct_color instances in two `hipcc -save-temps`
assembly files (symbol names and local label numbers aside):

    hipcc <the Makefile's HIPFLAGS> -save-temps -c csrc/jd_kernels.hip     # in each tree
    python tools/isa_diff.py OLD/jd_kernels-hip-amdgcn-amd-amdhsa-gfx950.s NEW/jd_kernels-hip-amdgcn-amd-amdhsa-gfx950.s

The bench measures these four instances (generic, 4:2:0, 4:2:2, 4:4:4 with interleaved RGB output): a
change to the colour/store stage's other formats must leave them instruction for instruction as they were.
Exits non-zero when one differs.
"""
import re
import sys


def instances(path):
    """layout index M -> instruction lines of k_idct_color<M> (format 0, or a tree without formats)."""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_ZN2jd12k_idct_colorILi(\d)(ELj(\d+))?E[^:]*):", line)
        if m:
            cur = int(m.group(2)) if m.group(4) in (None, "0") else None
            if cur is not None:
                out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].rstrip()
        if not t.strip() or (t.strip().startswith(".") and not t.startswith(".LBB")):
            continue  # comments, directives
        t = re.sub(r"_ZN2jd\w+", "SYM", t)
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main():
    a, b = instances(sys.argv[1]), instances(sys.argv[2])
    bad = 0
    for m in sorted(set(a) | set(b)):
        same = a.get(m) == b.get(m)
        bad += not same
        print(f"k_idct_color<{m}>: {len(a.get(m, []))} / {len(b.get(m, []))} lines, {'identical' if same else 'DIFFERENT'}")
    return 1 if bad or len(a) != 4 else 0


if __name__ == "__main__":
    sys.exit(main())
