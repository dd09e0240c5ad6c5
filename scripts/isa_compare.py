#!/usr/bin/env python
"""Do two source trees compile to the same gfx950 instructions?  Every translation unit of sugar_amd.build.SOURCES is compiled
from each tree to device assembly with the recipe's own flags (read from the FIRST tree's build.py) and the two texts are
compared; only the lines with the per-compilation `__hip_cuid_` symbol are left out.  The check for a refactor of kernel source:
every unit should print `same`, and whatever else prints is the whole difference.

    python scripts/isa_compare.py <tree A> <tree B>
"""
import difflib
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def recipe(tree):
    spec = importlib.util.spec_from_file_location("sgr_recipe", os.path.join(tree, "sugar_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(hipcc, flags, tree, src, out):
    csrc = os.path.join(tree, "sugar_amd", "csrc")
    r = subprocess.run([hipcc, *flags, f"-I{csrc}", "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src} of {tree}:\n{r.stdout}")
    return [l for l in open(out).read().splitlines() if "__hip_cuid_" not in l]


def main():
    a, b = (os.path.abspath(p) for p in sys.argv[1:3])
    rec = recipe(a)
    hipcc = rec._hipcc()
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        jobs = {src: [pool.submit(assembly, hipcc, rec.COMMON + extra, t, src, os.path.join(d, f"{i}_{src}.s")) for i, t in enumerate((a, b))]
                for src, extra in rec.SOURCES.items()}
        for src, (fa, fb) in jobs.items():
            diff = list(difflib.unified_diff(fa.result(), fb.result(), f"a/{src}", f"b/{src}", n=0, lineterm=""))
            print(f"{src}: same" if not diff else "\n".join(diff))


if __name__ == "__main__":
    main()
