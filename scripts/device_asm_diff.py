#!/usr/bin/env python3
"""Device-assembly comparison of every csrc/*.hip against another revision: the check of a refactor that must not move machine code.

    python scripts/device_asm_diff.py <base-rev> [-DNAME[=VALUE] ...]

Exports avmoe_amd/csrc and include of <base-rev> with `git archive` into a temporary directory, compiles every .hip file of that
tree and of the working tree to gfx950 assembly (the library's own flags, device side only, fixed compilation-unit id so that two
compilations of one file agree) and prints `identical` or the first differing lines per file.  Exit status 1 if any file differs
or exists on one side only.  Needs hipcc, no GPU."""
import difflib
import io
import os
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avmoe_amd.build import FLAGS, HIPCC  # noqa: E402

CSRC = os.path.join("avmoe_amd", "csrc")


def device_asm(tree, name, out, extra):
    """assembly lines of csrc/<name> in <tree>, or the compiler's message"""
    dst = os.path.join(out, name + ".s")
    cmd = [HIPCC] + [f for f in FLAGS if f != "-shared"] + extra + ["--cuda-device-only", "-S", "-cuid=fixed", os.path.join(tree, CSRC, name), "-o", dst]
    r = subprocess.run(cmd, cwd=out, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)   # cwd: the same relative context on both sides
    if r.returncode != 0:
        return ["hipcc failed:"] + r.stdout.splitlines()[:20]
    with open(dst) as fh:
        return fh.read().splitlines()


def main(argv):
    if not argv or argv[0].startswith("-"):
        sys.exit(__doc__)
    rev, extra = argv[0], argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "avmoe_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(base)
        sides = [(base, os.path.join(tmp, "a")), (ROOT, os.path.join(tmp, "b"))]
        names = [sorted(f for f in os.listdir(os.path.join(tree, CSRC)) if f.endswith(".hip")) for tree, _ in sides]
        for _, out in sides:
            os.makedirs(out)
        both = [n for n in names[0] if n in names[1]]
        with ThreadPoolExecutor(max_workers=8) as pool:             # at most 8 compilers at a time
            asm = [list(pool.map(lambda n: device_asm(tree, n, out, extra), both)) for tree, out in sides]
        bad = sorted(set(names[0]) ^ set(names[1]))
        for n in bad:
            print(f"{n}: only in {'the working tree' if n in names[1] else rev}")
        for n, a, b in zip(both, asm[0], asm[1]):
            if a == b and a[:1] != ["hipcc failed:"]:
                print(f"{n}: identical ({len(a)} lines)")
                continue
            bad.append(n)
            print(f"{n}: DIFFERENT")
            failed = [x for x in (a, b) if x[:1] == ["hipcc failed:"]]
            for line in failed[0] if failed else list(difflib.unified_diff(a, b, rev, "working tree", n=1, lineterm=""))[:24]:
                print("    " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
