"""Compare the gfx950 device assembly of every csrc/*.hip of the working tree with that of a git revision: the acceptance
check of a refactor that moves device code without changing it (the tap_common.h and tap_window.h moves).
REV is materialised with `git worktree add` under a temporary directory; both trees are compiled with the flags of
tests/test_kernel_asm_cpu.py (--cuda-device-only -S -O3 --offload-arch=gfx950).  What may legitimately differ is normalised away:
file paths, the compile-unit id (a hash of the source path), .file / .ident / .loc / .cfi / debug-section directives, and the
symbol renames named on the command line.  The comparison is of text only.
usage: python profiles/scripts/asm_vs_rev.py REV [-D MACRO ...] [--rename OLD=NEW ...] [--only conv_tap6.hip ...] [--keep DIR] [-j N]
exit status: 0 = every translation unit identical, 1 = at least one differs (or exists on one side only), 2 = a compile failed."""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join("multimodal-learning_amd", "csrc")
DROP = re.compile(r"^\s*\.(file|ident|loc|cfi_\w+|section\s+\.debug\S*)\b")


def compile_one(tree, name, out, defines):
    csrc = os.path.join(tree, CSRC)
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(tree, "include"), "-I" + csrc, "-Wno-unused-result",
           "--cuda-device-only", "-S"] + ["-D" + d for d in defines] + [os.path.join(csrc, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return name, r.returncode, r.stderr


def normalised(path, tree, renames):
    out = []
    for ln in open(path).read().split("\n"):
        if DROP.match(ln):
            continue
        ln = ln.replace(tree, "<tree>")
        ln = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", ln)
        for old, new in renames:
            ln = re.sub(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(old), new, ln)
        out.append(ln.rstrip())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="macro for both sides (PH_TAP_TRACE: the `make trace` variant)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="symbol of REV's text -> its name in the working tree")
    ap.add_argument("--only", nargs="+", default=None, help="translation units to compare (default: every csrc/*.hip of either tree)")
    ap.add_argument("--keep", default=None, metavar="DIR", help="keep the assembly texts under DIR/rev and DIR/tree")
    ap.add_argument("-j", "--jobs", type=int, default=16)
    ap.add_argument("--lines", type=int, default=12, help="differing lines printed per translation unit")
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    jobs = max(1, min(a.jobs, 16))

    tmp = tempfile.mkdtemp(prefix="asm_vs_rev_")
    rev_tree = os.path.join(tmp, "rev")
    outdir = a.keep or tmp
    status = 0
    try:
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", rev_tree, a.rev], check=True, capture_output=True, text=True)
        sides = {"rev": rev_tree, "tree": ROOT}
        names = {s: sorted(os.path.basename(f) for f in glob.glob(os.path.join(t, CSRC, "*.hip"))) for s, t in sides.items()}
        wanted = sorted(set(names["rev"]) | set(names["tree"]))
        if a.only:
            wanted = [n for n in wanted if n in a.only]
        for s in sides:
            os.makedirs(os.path.join(outdir, s), exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            futs = [pool.submit(compile_one, sides[s], n, os.path.join(outdir, s, n + ".s"), a.defines)
                    for n in wanted for s in sides if n in names[s]]
            failed = [(n, err) for n, rc, err in (f.result() for f in futs) if rc != 0]
        for n, err in failed:
            print("%s: compile failed\n%s" % (n, err[-2000:]))
        if failed:
            return 2
        for n in wanted:
            if n not in names["rev"] or n not in names["tree"]:
                print("%-20s only in %s" % (n, "the working tree" if n in names["tree"] else a.rev))
                status = 1
                continue
            old = normalised(os.path.join(outdir, "rev", n + ".s"), rev_tree, renames)
            new = normalised(os.path.join(outdir, "tree", n + ".s"), ROOT, [])
            if old == new:
                print("%-20s identical (%d lines)" % (n, len(new)))
                continue
            status = 1
            delta = [d for d in difflib.unified_diff(old, new, a.rev, "tree", n=0, lineterm="") if not d.startswith(("---", "+++"))]
            print("%-20s DIFFERS: %d lines removed, %d added" % (n, sum(d.startswith("-") for d in delta), sum(d.startswith("+") for d in delta)))
            for d in delta[:a.lines]:
                print("    " + d)
        return status
    finally:
        subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", rev_tree], capture_output=True)
        subprocess.run(["git", "-C", ROOT, "worktree", "prune"], capture_output=True)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
