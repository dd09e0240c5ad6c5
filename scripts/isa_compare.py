#!/usr/bin/env python
"""Do two source trees compile to the same gfx950 instructions?  Every translation unit of sugar_amd.build.SOURCES is compiled
from each tree to device assembly with the recipe's own flags (read from the FIRST tree's build.py) and the two texts are
compared; only the lines with the per-compilation `__hip_cuid_` symbol are left out.  The check for a refactor of kernel source:
every unit should print `same`, and whatever else prints is the whole difference.

    python scripts/isa_compare.py <tree A> <tree B>

A kernel that moves between units cannot be followed unit against unit.  `--by-kernel` compiles every unit of EACH tree's own
recipe, keys every kernel by its mangled name and compares per kernel: its instruction lines from its label to its `.Lfunc_end`
(trailing `;` comments and comment-only lines dropped, the function index of local labels normalised: `.LBB<f>_<n>` ->
`.LBB_<n>`) and its `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor block.  It prints `same` or the diff per kernel, the
names present in one tree only, and a one-line total.

    python scripts/isa_compare.py --by-kernel <tree A> <tree B>
"""
import difflib
import importlib.util
import os
import re
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


def kernels(lines):
    """{mangled name: (instruction lines, descriptor lines)} of one unit's assembly text"""
    desc = {}
    for i, l in enumerate(lines):
        if l.strip().startswith(".amdhsa_kernel "):
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            desc[l.split()[1]] = [x.strip() for x in lines[i:end + 1]]
    out = {}
    for name, d in desc.items():
        begin = next(j for j, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(j for j in range(begin, len(lines)) if lines[j].startswith(".Lfunc_end"))
        body = []
        for l in lines[begin + 1:end]:
            l = re.sub(r"\.LBB\d+_", ".LBB_", l.split(";", 1)[0]).rstrip()
            if l.strip():
                body.append(l)
        out[name] = (body, d)
    return out


def tree_kernels(pool, tree, d, tag):
    """{mangled name: (unit, instruction lines, descriptor lines)} over all units of the tree's own recipe"""
    rec = recipe(tree)
    hipcc = rec._hipcc()
    jobs = {src: pool.submit(assembly, hipcc, rec.COMMON + extra, tree, src, os.path.join(d, f"{tag}_{src}.s"))
            for src, extra in rec.SOURCES.items() if os.path.exists(os.path.join(tree, "sugar_amd", "csrc", src))}
    out = {}
    for src, job in jobs.items():
        for name, (body, desc) in kernels(job.result()).items():
            if name in out:
                raise RuntimeError(f"{tree}: kernel {name} is in {out[name][0]} and in {src}")
            out[name] = (src, body, desc)
    return out


def by_kernel(a, b):
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        ka, kb = tree_kernels(pool, a, d, "a"), tree_kernels(pool, b, d, "b")
    n_same = n_diff = 0
    for name in sorted(set(ka) & set(kb)):
        (ua, ia, da), (ub, ib, db) = ka[name], kb[name]
        where = ua if ua == ub else f"{ua} -> {ub}"
        diff = list(difflib.unified_diff(ia + da, ib + db, f"a/{ua}:{name}", f"b/{ub}:{name}", n=0, lineterm=""))
        if diff:
            n_diff += 1
            print("\n".join(diff))
        else:
            n_same += 1
            print(f"{name} [{where}]: same ({len(ia)} instruction lines)")
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    for name in only_a:
        print(f"only in a: {name} [{ka[name][0]}]")
    for name in only_b:
        print(f"only in b: {name} [{kb[name][0]}]")
    print(f"total: {n_same} same, {n_diff} different, {len(only_a)} only in a, {len(only_b)} only in b")
    return 0 if not (n_diff or only_a or only_b) else 1


def main():
    args = [x for x in sys.argv[1:] if x != "--by-kernel"]
    a, b = (os.path.abspath(p) for p in args[:2])
    if "--by-kernel" in sys.argv[1:]:
        sys.exit(by_kernel(a, b))
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
