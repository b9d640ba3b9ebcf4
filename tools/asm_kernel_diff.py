#!/usr/bin/env python3
"""Compare the kernels of two `hipcc -save-temps` assembly files function by function.

    tools/asm_kernel_diff.py OLD NEW [MAP]

OLD and NEW are each one assembly file or a directory: every `*.s` of a directory is read into one symbol table (kernels that moved between
translation units pair up by name; a symbol defined twice with different bodies is an error).
MAP, optional, is a file of `old_symbol=new_symbol` lines: a renamed instantiation is compared with its ancestor (and listed under its new name).

Per kernel symbol (a `.globl` function whose body ends at its `.Lfunc_end` label): the number of lines in each file and the number of
differing lines after local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...) are renumbered per function, so that a kernel added in front of another
does not show as a change.  Kernels present in one file only are listed with their register figures (from the .amdhsa_ directives and the
metadata comment block behind the body).  Exit status 1 when a kernel common to both files differs."""
import difflib
import glob
import os
import re
import sys

where = {}                                  # (directory, symbol) -> the file of the directory that defines it


def kernels(path):
    if os.path.isdir(path):                 # every *.s of the directory in one symbol table; `where` remembers each symbol's file for figures()
        out = {}
        for f in sorted(glob.glob(os.path.join(path, "*.s"))):
            for name, body in kernels(f).items():
                if name in out and normalise(out[name]) != normalise(body):
                    sys.exit(f"{name}: defined in {where[path, name]} and in {f} with different bodies")
                out[name] = body
                where[path, name] = f
        return out
    out, name, body = {}, None, []
    for line in open(path):
        s = line.rstrip("\n")
        m = re.match(r"^(_Z\w+):", s)
        if name is None and m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", s):
                out[name] = body
                name = None
                continue
            body.append(s)
    return out


def normalise(body):
    ids = {}

    def local(m):
        return ids.setdefault(m.group(0), f".L{len(ids)}")

    lines = []
    for s in body:
        s = s.split(";")[0].rstrip() if not s.lstrip().startswith(";") else ""
        if not s:
            continue
        lines.append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", local, s))
    return lines


def figures(path, name):
    text = open(where.get((path, name), path)).read()
    i = text.find(f".amdhsa_kernel {name}")
    blk = text[i:text.find(".end_amdhsa_kernel", i)] if i >= 0 else ""
    got = {}
    for key in ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size"):
        m = re.search(rf"\.amdhsa_{key} (\d+)", blk)
        if m:
            got[key] = int(m.group(1))
    j = text.find(f".name:           {name}")
    meta = text[j:j + 1500] if j >= 0 else ""
    for key in ("sgpr_spill_count", "vgpr_spill_count"):
        m = re.search(rf"\.{key}:\s+(\d+)", meta)
        if m:
            got[key] = int(m.group(1))
    return got


def main():
    old_p, new_p = sys.argv[1:3]
    old, new = kernels(old_p), kernels(new_p)
    if len(sys.argv) > 3:                   # MAP: lines `old_symbol=new_symbol`; such a kernel of OLD.s is compared under its new name
        renamed = dict(s.split("=") for s in open(sys.argv[3]).read().split())
        old = {renamed.get(k, k): v for k, v in old.items()}
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name in old and name in new:
            a, b = normalise(old[name]), normalise(new[name])
            nd = sum(1 for t in difflib.ndiff(a, b) if t[:1] in "+-") if a != b else 0
            print(f"{'same' if nd == 0 else 'DIFF'}  {len(a):6d} {len(b):6d} lines, {nd:5d} differing  {name}")
            bad += nd != 0
        else:
            which, p, body = ("old only", old_p, old.get(name)) if name in old else ("new only", new_p, new.get(name))
            body = normalise(body)
            n = lambda pat: sum(1 for s in body if re.search(pat, s))
            print(f"{which}  {len(body)} lines  {name}\n          {figures(p, name)}  mfma {n(r'v_mfma')}  v_cndmask {n(r'v_cndmask')}  "
                  f"v_readlane {n(r'v_readlane')}  v_writelane {n(r'v_writelane')}  scratch {n(r'scratch_')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
