#!/usr/bin/env python3
"""Diff of the DEVICE code of two builds of the kernel library, kernel by kernel.  No GPU needed.

    python tools/kernel_code_diff.py OLD NEW [--units boxes.hip,fgfa.hip] [--jobs 4] [--keep DIR]

OLD / NEW: a csrc directory (three levels below the include/ it uses), a git revision (its mega/pytorch_amd/csrc and
include/ are extracted), or `worktree`.

Every unit of build.SOURCES is compiled for the device alone (--cuda-device-only --no-gpu-bundle-output) with exactly
build.BASE_FLAGS plus the unit's own flags (the probed -mllvm flag included).  Per unit the report names
  * the kernel symbols present on one side only,
  * the kernels whose instruction encodings differ (llvm-objdump -d, compared by symbol, addresses dropped),
  * the kernels whose resource metadata differs (llvm-readelf --notes: registers, segment sizes, kernarg, workgroup).
A refactor of host code must come out as "identical" everywhere: the order of the kernels inside the code object may
change with the order of their first use on the host side, their code may not.  Exit status 1 if anything differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mega.pytorch_amd import build  # noqa: E402

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
CSRC_REL = "mega/pytorch_amd/csrc"
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
             "kernarg_segment_size", "max_flat_workgroup_size")


def resolve_tree(spec, tmp):
    """spec -> a directory holding the .hip / .h files."""
    if spec == "worktree":
        return os.path.join(ROOT, CSRC_REL)
    if os.path.isdir(spec):
        return os.path.abspath(spec)
    dst = os.path.join(tmp, "rev_" + re.sub(r"\W", "_", spec))
    os.makedirs(dst)
    # csrc/common.h includes ../../../include/mega_hip.h: a revision's header travels with its sources
    paths = [p for p in (CSRC_REL, "include")
             if subprocess.run(["git", "-C", ROOT, "cat-file", "-e", "%s:%s" % (spec, p)]).returncode == 0]
    tar = subprocess.run(["git", "-C", ROOT, "archive", spec] + paths, stdout=subprocess.PIPE, check=True).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return os.path.join(dst, CSRC_REL)


def compile_unit(csrc, unit, extra, out):
    cmd = [build.HIPCC] + build.BASE_FLAGS + extra + ["--cuda-device-only", "--no-gpu-bundle-output", "-c",
                                                      os.path.join(csrc, unit), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s" % (os.path.join(csrc, unit), r.stdout.decode()))


def kernel_metadata(obj):
    """{kernel symbol: {key: value}} from the code object's AMDGPU metadata note."""
    text = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", obj], stdout=subprocess.PIPE,
                          check=True).stdout.decode()
    kernels, cur, inside = {}, None, False
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line.startswith(" "):          # the next top-level key ends the list
            inside = False
            continue
        m = re.match(r"^  (-| ) \.(\w+):\s*(.*)$", line)   # keys of a kernel entry sit at this depth; .args' are deeper
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == "name":
            kernels[cur["name"]] = cur
    return {k: {key: v.get(key) for key in META_KEYS} for k, v in kernels.items()}


def kernel_encodings(obj, names):
    """{kernel symbol: tuple of instruction encodings}: the words llvm-objdump prints behind `// address:`, for the
    addresses inside the symbol's size (the zero padding up to the next symbol is not the kernel's)."""
    tool = lambda *a: subprocess.run([os.path.join(LLVM_BIN, a[0])] + list(a[1:]) + [obj], stdout=subprocess.PIPE,
                                     check=True).stdout.decode()
    end = {}
    for line in tool("llvm-readelf", "-sW").splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in names:
            end[f[7]] = int(f[1], 16) + int(f[2])
    enc, cur, limit = {}, None, 0
    for line in tool("llvm-objdump", "-d").splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = enc.setdefault(m.group(1), []) if m.group(1) in names else None
            limit = end.get(m.group(1), 0)
            continue
        if cur is None:
            continue
        m = re.search(r"//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)", line)
        if m and int(m.group(1), 16) < limit:
            cur.append(" ".join(m.group(2).split()))
    return {k: tuple(v) for k, v in enc.items()}


def describe(csrc, unit, extra, out):
    compile_unit(csrc, unit, extra, out)
    meta = kernel_metadata(out)
    return meta, kernel_encodings(out, set(meta))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--units", default="", help="comma-separated subset of build.SOURCES")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", default="", help="keep the device objects in this directory")
    a = ap.parse_args()
    units = [u for u in a.units.split(",") if u] or list(build.SOURCES)
    tmpctx = tempfile.TemporaryDirectory()
    tmp = a.keep or tmpctx.name
    os.makedirs(tmp, exist_ok=True)
    trees = [resolve_tree(a.old, tmpctx.name), resolve_tree(a.new, tmpctx.name)]
    flags = {u: (build._probe_flags(build.SOURCES[u]) if "-mllvm" in build.SOURCES[u] else list(build.SOURCES[u]))
             for u in units}
    with ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
        jobs = {(u, s): ex.submit(describe, trees[s], u, flags[u],
                                  os.path.join(tmp, "%s.%s.o" % (u[:-4], ("old", "new")[s])))
                for u in units for s in (0, 1) if os.path.exists(os.path.join(trees[s], u))}
        res = {k: f.result() for k, f in jobs.items()}
    total = same = 0
    dirty = False
    for u in units:
        if (u, 0) not in res or (u, 1) not in res:
            print("%-22s present on one side only" % u)
            dirty = True
            continue
        (m0, e0), (m1, e1) = res[(u, 0)], res[(u, 1)]
        only0, only1 = sorted(set(m0) - set(m1)), sorted(set(m1) - set(m0))
        both = sorted(set(m0) & set(m1))
        code = [k for k in both if e0.get(k) != e1.get(k)]
        meta = [k for k in both if m0[k] != m1[k]]
        total += len(both)
        same += len([k for k in both if k not in code and k not in meta])
        print("%-22s %3d kernels: %d only old, %d only new, %d code differs, %d metadata differs  [%s]" %
              (u, len(both), len(only0), len(only1), len(code), len(meta), " ".join(flags[u]) or "-"))
        for k in only0:
            print("    only old: %s" % k)
        for k in only1:
            print("    only new: %s" % k)
        for k in sorted(set(code) | set(meta)):
            print("    differs:  %s  (%d -> %d encodings)" % (k, len(e0.get(k, ())), len(e1.get(k, ()))))
            print("        old %s" % " ".join("%s=%s" % (key, m0[k][key]) for key in META_KEYS))
            print("        new %s" % " ".join("%s=%s" % (key, m1[k][key]) for key in META_KEYS))
        dirty = dirty or bool(only0 or only1 or code or meta)
    print("%d kernels on both sides, %d identical in code and metadata" % (total, same))
    return 1 if dirty else 0


if __name__ == "__main__":
    sys.exit(main())
