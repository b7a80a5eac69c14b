#!/usr/bin/env python3
"""Compare the compiled device code of two source trees kernel by kernel: for moves of kernels between translation units, which must not change them.

    python tools/kernel_isa_diff.py TREE_A TREE_B [--units-a gemm.hip] [--units-b gemm128.hip gemm256.hip ...] [--map OLD_KEY=NEW_KEY ...] [--keep DIR] [--jobs N]

Every unit of a tree is compiled with that tree's own `devias_amd.build._flags(unit) --cuda-device-only -S`, once as released and once with
-DDEVIAS_GEMM_DEBUG (units default to the tree's build.GEMM_SOURCES, or gemm.hip where a tree has no such list).  Kernels are keyed by their
name and (mangled) template arguments without namespaces and parameter types, so a kernel may change its unit, its namespace and the namespace of its parameter's type.
Per kernel it prints a verdict -- identical / differs (lines, and where: prologue = before the first MFMA, epilogue = behind the last, K loop = between) --
and requires equal descriptors (.amdhsa_* values: VGPR / AGPR / SGPR counts, LDS bytes, scratch) and equal MFMA counts.  Before the diff it drops comments and
.loc / .file / .ident lines and replaces what differs by construction: __hip_cuid_<hash>, mangled names, and the per-unit counters in local labels
(.LBB<n>_, .Lpost_getpc<n>, .Lfunc_end<n>, .Ltmp<n>).  It only normalises and diffs.  Exit status 1 if a kernel is missing or added, or a descriptor or MFMA count differs.
--map OLD_KEY=NEW_KEY (repeatable): a kernel of tree A whose key changed in tree B (a template parameter added or dropped) is compared with that successor
instead of being reported LOST / ADDED.
--keep DIR keeps the assembly there (DIR/a, DIR/b) and reuses files already present."""
import argparse
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(tree))), os.path.join(tree, "devias_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_unit(job):
    b, unit, debug, out = job
    if not os.path.exists(out):
        cmd = [b.HIPCC] + list(b._flags(unit)) + (["-DDEVIAS_GEMM_DEBUG"] if debug else []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, unit), "-o", out + ".tmp"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{unit}: {r.stderr[-2000:]}")
        os.replace(out + ".tmp", out)
    return open(out).read()


def key_of(mangled):
    """'_ZN12_GLOBAL__N_115gemm256p_kernelILb0ELi8EEEvN2ns1PE' -> 'gemm256p_kernelILb0ELi8EE': the kernel's name and its template arguments as mangled,
    without the enclosing namespaces and the parameter types (which name the namespace of the parameter's type)"""
    nested = mangled.startswith("_ZN")
    j = 3 if nested else 2
    while mangled[j].isdigit():            # the nested name's components, <length><identifier> each: the last one is the kernel
        m = re.match(r"\d+", mangled[j:])
        i = j + m.end()
        name, j = mangled[i:i + int(m.group())], i + int(m.group())
        if not nested:                     # an unnested name is ONE component: a digit behind it starts the first parameter's type (_Z18reduce_jobs_kernel10ReduceJobs)
            break
    if mangled[j:j + 1] != "I":
        return name
    depth, k = 0, j
    while True:                            # I ... E template argument list; L ... E literals and nested I ... E lists inside it
        depth += (mangled[k] in "IL") - (mangled[k] == "E")
        k += 1
        if depth == 0:
            return name + mangled[j:k]


def kernels_of(text):
    """{key: (body lines, descriptor dict, mfma count)} of one assembly file"""
    lines = text.split("\n")
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l.startswith("_Z") and l.split(":")[0] in names}
    out = {}
    for name in sorted(names):
        i = start[name]
        j = i
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        body, renum = [], {}
        for l in lines[i + 1:j + 1]:
            l = l.split(";")[0].rstrip()
            if not l.strip() or re.match(r"\s*\.(loc|file|ident)\b", l):
                continue
            l = re.sub(r"__hip_cuid_\w+", "__hip_cuid", l)
            l = re.sub(r"\b_Z\w+", lambda m: "KERNEL" if m.group(0) == name else "SYM", l)
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            l = re.sub(r"\.L(post_getpc|func_end|tmp)(\d+)", lambda m: ".L%s#%d" % (m.group(1), renum.setdefault(m.group(0), len(renum))), l)
            body.append(l.strip())
        k = text.index(".amdhsa_kernel " + name)
        desc = dict(re.findall(r"^\s*(\.amdhsa_\w+) (.+)$", text[k:text.index(".end_amdhsa_kernel", k)], re.M))
        del desc[".amdhsa_kernel"]
        desc = {f: re.sub(r"\b_Z\w+", "KERNEL", v) for f, v in desc.items()}        # (values may be expressions over the kernel's own symbols)
        for field, v in re.findall(r"^\s*\.set " + re.escape(name) + r"\.(\w+), (\S+)", text, re.M):
            if field in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size"):
                desc["." + field] = v
        out[key_of(name)] = (body, desc, sum("v_mfma" in l for l in body))
    return out


def where(a, b):
    """size and place of the difference between two bodies"""
    mf = [i for i, l in enumerate(a) if "v_mfma" in l]
    first, last = (mf[0], mf[-1]) if mf else (len(a), len(a))
    head = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    tail = next((i for i, (x, y) in enumerate(zip(reversed(a[head:]), reversed(b[head:]))) if x != y), min(len(a), len(b)) - head)
    places, n = set(), 0
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a[head:len(a) - tail], b[head:len(b) - tail], autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        n += max(i2 - i1, j2 - j1)
        places.add("prologue" if head + i2 <= first else ("epilogue" if head + i1 > last else "K loop"))
    return n, sorted(places)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a"); ap.add_argument("tree_b")
    ap.add_argument("--units-a", nargs="+"); ap.add_argument("--units-b", nargs="+")
    ap.add_argument("--map", action="append", default=[], metavar="OLD_KEY=NEW_KEY")
    ap.add_argument("--keep"); ap.add_argument("--jobs", type=int, default=min(int(os.environ.get("MAX_JOBS", 16)), os.cpu_count() or 4))
    args = ap.parse_args()
    tmp = None if args.keep else tempfile.TemporaryDirectory()
    root = args.keep or tmp.name
    trees = []
    for tag, tree, units in (("a", args.tree_a, args.units_a), ("b", args.tree_b, args.units_b)):
        b = load_build(os.path.abspath(tree))
        os.makedirs(os.path.join(root, tag), exist_ok=True)
        trees.append((tag, b, units or getattr(b, "GEMM_SOURCES", ["gemm.hip"])))
    bad = 0
    for debug in (False, True):
        jobs = [(b, u, debug, os.path.join(root, tag, u.replace(".hip", ".dbg.s" if debug else ".rel.s"))) for tag, b, units in trees for u in units]
        with ThreadPoolExecutor(args.jobs) as ex:
            texts = list(ex.map(compile_unit, jobs))
        na = len(trees[0][2])
        ka, kb = {}, {}
        for t in texts[:na]:
            ka.update(kernels_of(t))
        for old, new in (m.split("=", 1) for m in args.map):
            ka[new] = ka.pop(old)          # (a key that tree A does not have is an error)
        for t in texts[na:]:
            kb.update(kernels_of(t))
        print(f"==== {'-DDEVIAS_GEMM_DEBUG' if debug else 'release'}: {len(ka)} kernels in A, {len(kb)} in B")
        for k in sorted(set(ka) ^ set(kb)):
            print(f"  {'LOST ' if k in ka else 'ADDED'} {k}"); bad += 1
        same = 0
        for k in sorted(set(ka) & set(kb)):
            (a, da, ma), (b_, db, mb) = ka[k], kb[k]
            res = f"vgpr {da.get('.num_vgpr')} agpr {da.get('.num_agpr')} sgpr {da.get('.numbered_sgpr')} lds {da.get('.amdhsa_group_segment_fixed_size')} scratch {da.get('.private_seg_size')} mfma {ma} lines {len(a)}"
            if da != db:
                diff = {f: (da.get(f), db.get(f)) for f in sorted(set(da) | set(db)) if da.get(f) != db.get(f)}
                print(f"  DESCRIPTOR {k}: {diff}"); bad += 1
            if ma != mb:
                print(f"  MFMA COUNT {k}: {ma} -> {mb}"); bad += 1
            if a == b_:
                same += 1
                print(f"  identical  {k}: {res}")
            else:
                n, places = where(a, b_)
                print(f"  differs    {k}: {n} lines in {', '.join(places)}; {res}")
        print(f"  {same} of {len(set(ka) & set(kb))} common kernels identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
