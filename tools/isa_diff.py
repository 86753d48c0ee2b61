#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, translation unit by translation unit.

    python tools/isa_diff.py <tree A> <tree B>

Every mm_dfn_amd/csrc/*.hip of each tree is compiled device-only to assembly with the flags of mm_dfn_amd/build.py, once plain
and once with -DMMDFN_TUNING, into a temporary directory.  Lines containing ``__hip_cuid_`` (a per-compile symbol) are dropped
and the rest is compared as text: per file and build the tool prints ``identical`` or the number of differing lines, and it
exits non-zero on any difference.  A refactor that leaves every line identical runs the parent's kernels.
"""
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ARCH = "gfx950"
JOBS = 16
BUILDS = (("production", []), ("tuning", ["-DMMDFN_TUNING"]))


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise SystemExit("hipcc not found")
    return exe


def sources(tree):
    csrc = os.path.join(tree, "mm_dfn_amd", "csrc")
    return {f: os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}


def compile_asm(job):
    tree, src, defs, out = job
    cmd = [hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(tree, "include")]
    cmd += defs + ["--cuda-device-only", "-S", src, "-o", out]
    proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stderr)
        raise SystemExit("compile failed: " + " ".join(cmd))


def asm_lines(path):
    with open(path) as fh:
        lines = [line for line in fh if "__hip_cuid_" not in line]
    with open(path, "w") as fh:
        fh.writelines(lines)
    return lines


def differing_lines(a, b):
    out = subprocess.run(["diff", a, b], stdout=subprocess.PIPE, text=True).stdout
    return sum(1 for d in out.splitlines() if d[:1] in "<>")


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    trees = [os.path.abspath(t) for t in argv[1:]]
    srcs = [sources(t) for t in trees]
    bad = 0
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        jobs = []
        for side, (tree, files) in enumerate(zip(trees, srcs)):
            for build, defs in BUILDS:
                os.makedirs(os.path.join(tmp, str(side), build))
                for name, src in files.items():
                    jobs.append((tree, src, defs, os.path.join(tmp, str(side), build, name[:-4] + ".s")))
        with ThreadPoolExecutor(JOBS) as pool:
            list(pool.map(compile_asm, jobs))
        for name in sorted(set(srcs[0]) | set(srcs[1])):
            for build, _ in BUILDS:
                if name not in srcs[0] or name not in srcs[1]:
                    print("%-24s %-10s only in %s" % (name, build, trees[0] if name in srcs[0] else trees[1]))
                    bad += 1
                    continue
                pa, pb = (os.path.join(tmp, str(side), build, name[:-4] + ".s") for side in (0, 1))
                a, b = asm_lines(pa), asm_lines(pb)
                if a == b:
                    print("%-24s %-10s identical (%d lines)" % (name, build, len(a)))
                else:
                    print("%-24s %-10s %d differing lines" % (name, build, differing_lines(pa, pb)))
                    bad += 1
    print("all identical" if not bad else "%d of %d comparisons differ" % (bad, 2 * len(set(srcs[0]) | set(srcs[1]))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
