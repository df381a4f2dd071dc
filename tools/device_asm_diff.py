#!/usr/bin/env python3
"""Device code of two trees of this repository, compared function by function.

    python tools/device_asm_diff.py <tree A> <tree B> [--jobs N] [--work DIR]

The check for an edit that is meant to leave the device code alone (moving
definitions between headers, renaming a file, rewording a comment): compile
every madigan_amd/csrc/*.hip and tests/csrc/mgn_math_probe.hip of both trees
to gfx950 assembly, with each tree's own build.FLAGS and build.unit_flags(),
and compare the text per symbol -- per kernel and per non-inlined device
function, not per file, because moving a definition may reorder the
non-inlined helpers.  A kernel's .amdhsa_* block and its metadata entry are
part of its text.  No GPU, no third-party module.

Prints per unit the number of functions compared and the names of those that
differ, are missing from B or are new in B; exits 1 if there are any.  --work
keeps the assembly (DIR/a, DIR/b) for a look at what differs.

It only diffs text: it knows nothing about particular instructions.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

# without a fixed compilation-unit id the __hip_cuid_<hash> symbol hashes the
# source's path, and two copies of one tree differ
CUID = "-cuid=0"
PROBE = os.path.join("tests", "csrc", "mgn_math_probe.hip")


def load_build(tree):
    """The tree's own madigan_amd/build.py, without importing the package."""
    path = os.path.join(tree, "madigan_amd", "build.py")
    spec = importlib.util.spec_from_file_location("_mgn_build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def commands(tree, outdir):
    """[(unit name, command)]: one device-only -S compile per unit."""
    b = load_build(tree)
    csrc = os.path.join(tree, "madigan_amd", "csrc")
    srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip"))
    srcs.append(os.path.join(tree, PROBE))
    out = []
    for src in srcs:
        unit = os.path.basename(src)
        out.append((unit, [b.hipcc(), *b.FLAGS, *b.unit_flags(unit), f"-I{csrc}",
                           f"-I{os.path.join(tree, 'include')}", "--cuda-device-only", "-S", CUID,
                           "-o", os.path.join(outdir, unit[:-4] + ".s"), src]))
    return out


def compile_all(cmds, jobs):
    def one(uc):
        r = subprocess.run(uc[1], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed: {' '.join(uc[1])}\n{r.stderr}")
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, cmds))


_SYM = re.compile(r"^\t\.type\t([^,\s]+),@(function|object)")
# lines the assembler prints ahead of a symbol's .type: they belong to it
_LEAD = re.compile(r"^\t\.(section|text|protected|globl|weak|hidden|p2align)\b")
# a function's position in the file is part of its local labels
_LOCAL = re.compile(r"(\.L(?:BB|func_begin|func_end|JTI|CPI))\d+(_\d+)?\b")
_MD_ENTRY = re.compile(r"^  - ")
_MD_NAME = re.compile(r"^    \.name:\s+(\S+)")


def split_symbols(text):
    """{key: [lines]} with key 'function <sym>' / 'object <sym>', the kernels'
    metadata entries appended to their functions, and what belongs to no
    symbol under '(preamble)' and '(metadata)'."""
    lines = text.splitlines()
    md0 = next((i for i, ln in enumerate(lines) if ln.strip() == ".amdgpu_metadata"), len(lines))
    chunks, key, start = {}, "(preamble)", 0
    for i in range(md0):
        m = _SYM.match(lines[i])
        if not m:
            continue
        cut = i
        while cut > start and _LEAD.match(lines[cut - 1]):
            cut -= 1
        chunks.setdefault(key, []).extend(lines[start:cut])
        key, start = f"{m.group(2)} {m.group(1)}", cut
    chunks.setdefault(key, []).extend(lines[start:md0])
    rest, entry = [], None
    for ln in lines[md0:]:
        if _MD_ENTRY.match(ln):
            if entry:
                _file_entry(chunks, rest, entry)
            entry = [ln]
        elif entry is not None and ln.startswith("    "):
            entry.append(ln)
        else:
            if entry:
                _file_entry(chunks, rest, entry)
            entry = None
            rest.append(ln)
    chunks["(metadata)"] = rest
    return {k: [_LOCAL.sub(r"\1\2", ln) for ln in v] for k, v in chunks.items()}


def _file_entry(chunks, rest, entry):
    name = next((m.group(1) for m in map(_MD_NAME.match, entry) if m), None)
    (chunks.setdefault(f"function {name}", []) if name else rest).extend(entry)


def compare_unit(path_a, path_b):
    """(functions compared, [differing], [missing from B], [new in B])."""
    with open(path_a) as f:
        a = split_symbols(f.read())
    with open(path_b) as f:
        b = split_symbols(f.read())
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    missing = sorted(k for k in a if k not in b)
    new = sorted(k for k in b if k not in a)
    return sum(k.startswith("function ") for k in a if k in b), differ, missing, new


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--work", help="keep the assembly under this directory")
    args = ap.parse_args(argv)
    work = args.work or tempfile.mkdtemp(prefix="device_asm_diff_")
    dirs = [os.path.join(work, d) for d in ("a", "b")]
    cmds = []
    for tree, d in zip((args.tree_a, args.tree_b), dirs):
        os.makedirs(d, exist_ok=True)
        cmds += commands(os.path.abspath(tree), d)
    compile_all(cmds, args.jobs)
    bad = report(*dirs)
    if not args.work:
        import shutil
        shutil.rmtree(work)
    return 1 if bad else 0


def report(dir_a, dir_b):
    """Print the comparison of two directories of assembly; the number of
    symbols that differ, are missing or are new."""
    bad = total = 0
    units_a, units_b = (sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in (dir_a, dir_b))
    for u in sorted(set(units_a) | set(units_b)):
        if u not in units_a or u not in units_b:
            print(f"{u[:-2]}: unit {'missing from B' if u in units_a else 'new in B'}")
            bad += 1
            continue
        n, differ, missing, new = compare_unit(os.path.join(dir_a, u), os.path.join(dir_b, u))
        total += n
        bad += len(differ) + len(missing) + len(new)
        print(f"{u[:-2]}: {n} functions compared, {len(differ)} differ, {len(missing)} missing, {len(new)} new")
        for label, names in (("differs", differ), ("missing from B", missing), ("new in B", new)):
            for k in names:
                print(f"    {label}: {k}")
    print(f"total: {total} functions compared, {bad} symbols differ, are missing or are new")
    return bad


if __name__ == "__main__":
    sys.exit(main())
