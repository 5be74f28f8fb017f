#!/usr/bin/env python3
"""Do two source trees compile to the same GPU kernels?

    tools/kernel_diff.py A/csrc B/csrc [--only FILE ...]

Compiles every .hip file of both csrc/ directories to device assembly only
(build.py's compiler, arch and flags; no host pass, nothing is linked or run)
and compares the two trees function by function, keyed by mangled name
WHICHEVER FILE the function sits in -- so a kernel that moved to another
translation unit is compared with itself.  The text compared is the
function's instructions: comments and directives are dropped and local labels
are renumbered in order of appearance.  Per kernel it prints `same` or
`differs` and the kernel's VGPRs, AGPRs, SGPRs (the code object's metadata),
private-segment (scratch) bytes and static LDS bytes (its kernel descriptor);
a change in any of these counts as a difference.  The named device data
objects (the __constant__ tables and scalar constants the kernels address by
symbol) are compared by name, size and initialiser.

Exit status 1 when a function or object differs, is missing from B, or is new
in B; 0 otherwise.  --only FILE ... limits both trees to the files of those
names (a kernel that moved out of them then shows as missing).

It diffs two texts; it looks for no particular instruction.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from collections import defaultdict
from pathlib import Path

# build.py's flags (build(): the release flags; -Xarch_host is the host pass's)
FLAGS = ["-O3", "-Wno-unused-result", "-Wno-pass-failed", "-pthread", "-Xarch_host", "-march=x86-64-v3"]
RES = ("vgpr", "agpr", "sgpr", "scratch", "lds")


def build_settings(csrc: Path):
    """HIPCC and ARCH as the tree's build.py states them."""
    spec = importlib.util.spec_from_file_location("bpp_build", csrc.parent / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, mod.ARCH


def compile_asm(hipcc: str, arch: str, src: Path, out: Path) -> str:
    cmd = [hipcc, f"--offload-arch={arch}", "-fPIC", "-std=c++17", *FLAGS, "--cuda-device-only", "-S", "-x", "hip",
           str(src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=src.parent)
    if r.returncode != 0:
        raise RuntimeError(f"compile failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return out.read_text()


_LABEL = re.compile(r"\.L[A-Za-z_$][\w$.]*")


def normalise(lines):
    """Instruction text of one function: no comments, no directives, local
    labels numbered by first appearance."""
    names: dict[str, str] = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln or (ln.startswith(".") and not ln.endswith(":")):
            continue
        ln = _LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), ln)
        out.append(re.sub(r"\s+", " ", ln))
    return "\n".join(out)


def parse(text: str):
    """-> functions {name: instruction text}, resources {kernel: {..}},
    objects {name: (size, initialiser text)}"""
    lines = text.split("\n")
    kind = {}
    for ln in lines:
        m = re.match(r"\s*\.type\s+([^\s,]+),@(function|object)", ln)
        if m:
            kind[m.group(1)] = m.group(2)
    funcs, objs, res = {}, {}, defaultdict(dict)
    i = 0
    while i < len(lines):
        m = re.match(r"([^\s:;]+):", lines[i])
        name = m.group(1) if m else None
        if name and kind.get(name) == "function":
            j = i + 1
            while j < len(lines) and not re.match(r"\s*\.Lfunc_end\d+:", lines[j]):
                j += 1
            body = lines[i + 1:j]
            # the kernel descriptor sits inside the function's span: read it, keep it out of the text
            for ln in body:
                for key, tag in (("private_segment", "scratch"), ("group_segment", "lds")):
                    d = re.match(rf"\s*\.amdhsa_{key}_fixed_size\s+(\d+)", ln)
                    if d:
                        res[name][tag] = int(d.group(1))
            funcs[name] = normalise(body)
            i = j
        elif name and kind.get(name) == "object" and not name.startswith("__hip_cuid_"):  # (the unit's id: a hash)
            j = i + 1
            init = []
            while j < len(lines) and not re.match(rf"\s*\.size\s+{re.escape(name)},", lines[j]):
                init.append(re.sub(r"\s+", " ", lines[j].split(";", 1)[0].strip()))
                j += 1
            size = lines[j].split(",", 1)[1].strip() if j < len(lines) else "?"
            objs[name] = (size, "\n".join(x for x in init if x))
            i = j
        i += 1
    # registers: the metadata note (one YAML map per kernel)
    meta = text.split(".amdgpu_metadata", 1)
    if len(meta) == 2:
        for entry in re.split(r"\n\s+- \.agpr_count:", "\n" + meta[1])[1:]:
            entry = ".agpr_count:" + entry
            nm = re.search(r"\.name:\s+(\S+)", entry)
            if not nm:
                continue
            for key, tag in ((".vgpr_count", "vgpr"), (".agpr_count", "agpr"), (".sgpr_count", "sgpr")):
                v = re.search(rf"{re.escape(key)}:\s+(\d+)", entry)
                if v:
                    res[nm.group(1).strip("'\"")][tag] = int(v.group(1))
    return funcs, dict(res), objs


def tree(csrc: Path, only, tmp: Path, jobs: int):
    hipcc, arch = build_settings(csrc)
    srcs = sorted(p for p in csrc.glob("*.hip") if not only or p.name in only)
    if not srcs:
        raise SystemExit(f"{csrc}: no .hip file to compile")
    tmp.mkdir(parents=True, exist_ok=True)
    with cf.ThreadPoolExecutor(jobs) as ex:
        texts = list(ex.map(lambda s: compile_asm(hipcc, arch, s, tmp / (s.name + ".s")), srcs))
    funcs, res, objs = defaultdict(list), {}, defaultdict(list)  # name -> [(file, text)] (one copy per unit)
    for s, t in zip(srcs, texts):
        f, r, o = parse(t)
        for k, v in f.items():
            funcs[k].append((s.name, v))
        for k, v in o.items():
            objs[k].append((s.name, v))
        for k, v in r.items():
            res.setdefault(k, []).append(v)
    return funcs, res, objs


def compare(what, a, b, ra=None, rb=None):
    bad = 0
    for name in sorted(set(a) | set(b)):
        files = ",".join(sorted({f for f, _ in b.get(name, a.get(name))}))
        if name not in b:
            print(f"missing  {what} {name}  [{files}]")
            bad += 1
            continue
        if name not in a:
            print(f"new      {what} {name}  [{files}]")
            bad += 1
            continue
        # (a name defined in several units -- an internal constant, one copy each -- as the set of its texts)
        same = {t for _, t in a[name]} == {t for _, t in b[name]}
        note = ""
        if ra is not None and name in rb:
            xa, xb = ra.get(name, [{}]), rb[name]
            cols = []
            for tag in RES:
                va, vb = sorted({r.get(tag) for r in xa}, key=str), sorted({r.get(tag) for r in xb}, key=str)
                cols.append(f"{tag} {'/'.join(map(str, vb))}" if va == vb else
                            f"{tag} {'/'.join(map(str, va))} -> {'/'.join(map(str, vb))}")
                same = same and va == vb
            note = "  " + "  ".join(cols)
        elif what == "object":
            note = "  " + "/".join(sorted({f"{v[0]} B" for _, v in b[name]}))
        print(f"{'same   ' if same else 'differs'}  {what} {name}  [{files}]{note}")
        bad += not same
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", type=Path, help="the first tree's csrc/ (the parent's)")
    ap.add_argument("b", type=Path, help="the second tree's csrc/")
    ap.add_argument("--only", nargs="+", default=[], metavar="FILE", help="compile only the .hip files of these names")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 4))
    ap.add_argument("--keep", type=Path, default=None, help="keep the assembly files under this directory")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        root = a.keep or Path(td)
        fa, ra, oa = tree(a.a.resolve(), set(a.only), root / "a", a.jobs)
        fb, rb, ob = tree(a.b.resolve(), set(a.only), root / "b", a.jobs)
    kernels = lambda f, r: {k: v for k, v in f.items() if k in r}
    others = lambda f, r: {k: v for k, v in f.items() if k not in r}
    bad = compare("kernel", kernels(fa, ra), kernels(fb, rb), ra, rb)
    bad += compare("function", others(fa, ra), others(fb, rb))
    bad += compare("object", oa, ob)
    nk = len(kernels(fb, rb))
    print(f"{nk} kernels, {len(others(fb, rb))} other functions, {len(ob)} objects in B: " +
          ("all the same as A" if not bad else f"{bad} differ, are missing or are new"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
