#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two csrc directories, file by file.

    git worktree add /tmp/parent HEAD~1
    python tools/isa_diff.py /tmp/parent/<package>/csrc <package>/csrc [name.hip ...]

Every .hip of both directories (or only the named ones) is compiled from inside its own
directory with that directory's Makefile HIPFLAGS plus --offload-device-only -S. The two texts
are compared after dropping the lines that carry the __hip_cuid_ symbol, which hashes the
source text and so differs for any edit. Per file: the kernel count and "identical", or the
first differing line. Exit status 1 if any file differs. Needs hipcc, no GPU.
"""
import argparse
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

JOBS = 16


def make_var(makefile, name, env):
    m = re.search(rf"^{name}\s*\??=\s*(.*)$", makefile, re.M)
    if not m:
        sys.exit(f"no {name} in Makefile")
    return re.sub(r"\$\((\w+)\)", lambda v: env[v.group(1)], m.group(1).strip())


def compile_cmd(csrc):
    mk = (csrc / "Makefile").read_text()
    env = {"ARCH": make_var(mk, "ARCH", {})}
    return [make_var(mk, "HIPCC", env)] + make_var(mk, "HIPFLAGS", env).split() + ["--offload-device-only", "-S"]


def assemble(job):
    csrc, name, out = job
    r = subprocess.run(compile_cmd(csrc) + [name, "-o", str(out)], cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        return r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "hipcc failed"
    return None


def isa_lines(path):
    return [l for l in path.read_text().splitlines() if "__hip_cuid_" not in l]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", type=Path, help="csrc directory of the parent")
    ap.add_argument("b", type=Path, help="csrc directory of the branch")
    ap.add_argument("names", nargs="*", help="restrict to these .hip files")
    args = ap.parse_args()
    a, b = args.a.resolve(), args.b.resolve()
    in_a, in_b = ({p.name for p in d.glob("*.hip")} for d in (a, b))
    names = sorted(args.names or in_a | in_b)

    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        jobs = [(d, n, tmp / f"{tag}_{n}.s") for n in names for tag, d, have in (("a", a, in_a), ("b", b, in_b)) if n in have]
        with ThreadPoolExecutor(JOBS) as pool:
            errors = dict(zip(((j[0], j[1]) for j in jobs), pool.map(assemble, jobs)))
        for n in names:
            if n not in in_a or n not in in_b:
                print(f"{n}: only in {'b' if n in in_b else 'a'}")
                differ += 1
                continue
            err = errors[(a, n)] or errors[(b, n)]
            if err:
                print(f"{n}: compile error: {err}")
                differ += 1
                continue
            la, lb = isa_lines(tmp / f"a_{n}.s"), isa_lines(tmp / f"b_{n}.s")
            kernels = sum(l.lstrip().startswith(".amdhsa_kernel ") for l in lb)
            if la == lb:
                print(f"{n}: {kernels} kernels, {len(lb)} lines, identical")
                continue
            differ += 1
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"{n}: {kernels} kernels, DIFFERS at line {i + 1} ({len(la)} vs {len(lb)} lines)")
            print(f"  a: {la[i] if i < len(la) else '<end>'}")
            print(f"  b: {lb[i] if i < len(lb) else '<end>'}")
    print(f"{len(names) - differ} of {len(names)} files identical")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
