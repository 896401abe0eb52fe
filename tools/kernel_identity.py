#!/usr/bin/env python3
"""Are the compiled kernels of two source trees the same?  (CPU only: hipcc cross-compiles, nothing runs.)

Every listed .hip file is compiled to gfx950 assembly in both trees, with the flags of the tree's csrc/Makefile
(per-file additions included) plus `--offload-device-only -S -Rpass-analysis=kernel-resource-usage`.  Kernels are
matched by mangled name ACROSS files, so a kernel may move from one file to another.  Compared as plain text:

* resources: .vgpr_count, .agpr_count, .sgpr_count, .private_segment_fixed_size (scratch) and
  .group_segment_fixed_size (static LDS) of the kernel's metadata, and the occupancy of the resource-usage remark;
* instruction stream: every line of the kernel's body, labels included, with comments and .loc / .file / .ident /
  .cfi / .p2align / .section lines removed.  The one normalisation: a local label carries the ordinal of its
  function inside the file (.LBB7_3), which changes when a kernel moves, so the ordinal is dropped (.LBB_3).

    python tools/kernel_identity.py OLD_TREE NEW_TREE --old-files conv3d.hip --new-files conv3d_igemm.hip conv3d_halo.hip
    python tools/kernel_identity.py OLD_TREE NEW_TREE --files vae.hip unet.hip          # the same names in both trees

A kernel that was renamed is matched with --map OLD=NEW: OLD and NEW are substrings of the mangled name, and every old
kernel whose name contains OLD is compared under the name with NEW in its place (the template arguments and the signature
are part of the mangled name, so a rename that changes them needs them inside OLD and NEW):

    python tools/kernel_identity.py OLD_TREE NEW_TREE --files attention.hip --map 23set_attention_om_kernelILi32EE=28set_attention_generic_kernelILi32ELNS_11AttnSoftmaxE1EE

File names are relative to <tree>/3d-shape-generation_amd/csrc.  Exit status 0: the two sets of kernels are equal and
every kernel is identical; 1 otherwise.  --markdown prints the outcome as a table row per file.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("3d-shape-generation_amd", "csrc")
RESOURCE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
DROPPED = (".loc", ".file", ".ident", ".cfi", ".p2align", ".section")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+_(\d+)")


def makefile_flags(tree, name):
    """CXXFLAGS of the tree's Makefile for one source file, $(ARCH) resolved."""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).split()
    obj = re.escape(os.path.splitext(name)[0] + ".o")
    for extra in re.findall(r"^" + obj + r"\s*:\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M):
        flags += extra.split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    return hipcc, [f.replace("$(ARCH)", arch) for f in flags]


def compile_file(tree, name, outdir):
    hipcc, flags = makefile_flags(tree, name)
    out = os.path.join(outdir, name + ".s")
    cmd = [hipcc] + flags + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", name, "-o", out]
    res = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed in {tree}:\n{res.stderr[-3000:]}")
    return open(out).read(), res.stderr


def kernels_of(asm, remarks):
    """{mangled name: {"body": [lines], "res": {key: value}}} of one compiled file."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    lines = asm.split("\n")
    start = {}
    for i, line in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in names:
            start[m.group(1)] = i
    out = {}
    for name in names:
        body = []
        for line in lines[start[name] + 1:]:
            if re.match(r"^\.Lfunc_end\d+:", line):
                break
            line = line.split(";", 1)[0].strip()
            if not line or line.startswith(DROPPED):
                continue
            body.append(LOCAL_LABEL.sub(r".L\1_\2", " ".join(line.split())))
        out[name] = {"body": body, "res": {}}
    # metadata: one YAML map per kernel, `  - .agpr_count:` opens it
    # (the split eats the "  - " in front of the first key, .agpr_count, which then starts at column 0)
    for block in re.split(r"^  - (?=\.agpr_count:)", asm, flags=re.M)[1:]:
        fields = dict(re.findall(r"^\s{0,4}(\.\w+):\s+(\S+)\s*$", block, re.M))
        if fields.get(".name") in out:
            out[fields[".name"]]["res"].update({k: fields[k] for k in RESOURCE_KEYS if k in fields})
    cur = None
    for line in remarks.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur in out:
            out[cur]["res"]["occupancy"] = m.group(1)
    for name, k in out.items():             # a figure that was not found must not compare equal to another that was not found
        missing = [key for key in RESOURCE_KEYS + ("occupancy",) if k["res"].get(key) is None]
        if missing or not k["body"]:
            raise RuntimeError(f"{name}: could not read {', '.join(missing) or 'the instruction stream'} from the compiler's output")
    return out


def tree_kernels(tree, files, jobs):
    found = {}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for name, (asm, remarks) in zip(files, pool.map(lambda f: compile_file(tree, f, tmp), files)):
            for k, v in kernels_of(asm, remarks).items():
                if k in found:
                    raise RuntimeError(f"{k} is defined in {found[k]['file']} and in {name}")
                found[k] = dict(v, file=name)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--files", nargs="+", default=[], help="files compiled in both trees")
    ap.add_argument("--old-files", nargs="+", default=[], help="files compiled in the old tree only")
    ap.add_argument("--new-files", nargs="+", default=[], help="files compiled in the new tree only")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW",
                    help="a renamed kernel: the substring OLD of an old tree's mangled name reads NEW (may be given several times)")
    a = ap.parse_args()
    old = tree_kernels(a.old_tree, a.files + a.old_files, a.jobs)
    new = tree_kernels(a.new_tree, a.files + a.new_files, a.jobs)
    for rule in a.map:
        frm, sep, to = rule.partition("=")
        if not sep or not frm:
            ap.error(f"--map {rule}: expected OLD=NEW")
        hits = [k for k in old if frm in k]
        if not hits:
            ap.error(f"--map {rule}: no kernel of the old tree has {frm} in its name")
        for k in hits:
            renamed = k.replace(frm, to)
            if renamed in old:
                ap.error(f"--map {rule}: {k} would become {renamed}, which the old tree already has")
            print(f"MAPPED {k} -> {renamed}")
            old[renamed] = old.pop(k)
            old[renamed]["body"] = [line.replace(k, renamed) for line in old[renamed]["body"]]   # (its own name in its directives)
    bad = 0
    for k in sorted(set(old) - set(new)):
        print(f"LOST   {k} ({old[k]['file']})")
        bad += 1
    for k in sorted(set(new) - set(old)):
        print(f"ADDED  {k} ({new[k]['file']})")
        bad += 1
    per_file = {}
    for k in sorted(set(old) & set(new)):
        o, n = old[k], new[k]
        same = True
        if o["res"] != n["res"]:
            print(f"RESOURCES differ: {k}\n  old {o['file']}: {o['res']}\n  new {n['file']}: {n['res']}")
            same = False
        if o["body"] != n["body"]:
            i = next((i for i, (x, y) in enumerate(zip(o["body"], n["body"])) if x != y), min(len(o["body"]), len(n["body"])))
            print(f"STREAM differs: {k} ({len(o['body'])} / {len(n['body'])} lines), first at line {i}:\n"
                  f"  old: {o['body'][i] if i < len(o['body']) else '<end>'}\n  new: {n['body'][i] if i < len(n['body']) else '<end>'}")
            same = False
        bad += 0 if same else 1
        row = per_file.setdefault((o["file"], n["file"]), [0, 0, 0])
        row[0] += 1
        row[1] += 1 if same else 0
        row[2] += len(n["body"])
    if a.markdown:
        print("| old file | new file | kernels | identical | lines compared |\n|---|---|---|---|---|")
        for (fo, fn), (cnt, same, nl) in sorted(per_file.items()):
            print(f"| `{fo}` | `{fn}` | {cnt} | {same} | {nl} |")
    print(f"{len(old)} kernels in the old tree, {len(new)} in the new one, {len(set(old) & set(new))} matched by name, "
          f"{'all identical' if bad == 0 else str(bad) + ' NOT identical / lost / added'}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
