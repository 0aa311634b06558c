#!/usr/bin/env python3
"""Is the device code of two source trees the same?  For a refactor that must not change a kernel.

    python tools/device_asm_diff.py PARENT_CSRC TREE_CSRC [NAME.hip ...]

Every *.hip present in both csrc directories (or only the named ones) is compiled device-only to gfx950 assembly with the flags of
resselt_amd/build.py (compile_command), in each tree with that tree's own headers.  Lines naming __hip_cuid_ (a hash of the source
text) are dropped, as is the `.file` line; one line per file says IDENTICAL or shows the first differing line.  Exit status 1 on any
difference.  Runs without a GPU, at most 16 compilations at a time.
"""

from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from resselt_amd.build import ROOT, compile_command  # noqa: E402


def device_asm(hipcc: str, csrc: str, name: str, tmp: str, tag: str) -> list[str]:
    include = os.path.normpath(os.path.join(csrc, '..', '..', 'include'))
    if not os.path.exists(os.path.join(include, 'resselt_amd.h')):
        include = os.path.join(ROOT, 'include')
    out = os.path.join(tmp, f'{tag}_{name}.s')
    cmd = compile_command(hipcc, os.path.join(csrc, name), out, csrc=csrc, include=include)
    cmd[cmd.index('-c')] = '-S'
    cmd[1:1] = ['--cuda-device-only', '-Wno-unused-command-line-argument']
    subprocess.run(cmd, check=True)
    with open(out, encoding='utf-8', errors='replace') as fh:
        lines = [ln.rstrip('\n') for ln in fh if '__hip_cuid_' not in ln and not ln.lstrip().startswith('.file')]
    os.remove(out)
    return lines


def compare(job) -> tuple[str, str]:
    hipcc, parent, tree, name, tmp = job
    a, b = device_asm(hipcc, parent, name, tmp, 'a'), device_asm(hipcc, tree, name, tmp, 'b')
    if a == b:
        return name, f'IDENTICAL ({len(a)} lines)'
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return name, f'DIFFERENT at line {i + 1}:\n    parent: {x.strip()}\n    tree:   {y.strip()}'
    return name, f'DIFFERENT: {len(a)} lines in the parent, {len(b)} in the tree, the shorter is a prefix of the longer'


def main(argv) -> int:
    if len(argv) < 2:
        print(__doc__)
        return 2
    parent, tree = os.path.abspath(argv[0]), os.path.abspath(argv[1])
    names = sorted(f for f in os.listdir(parent) if f.endswith('.hip') and os.path.exists(os.path.join(tree, f)))
    if argv[2:]:
        names = [n for n in names if n in argv[2:]]
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:
        bad = 0
        for name, verdict in pool.map(compare, [(hipcc, parent, tree, n, tmp) for n in names]):
            print(f'{name}: {verdict}', flush=True)
            bad += not verdict.startswith('IDENTICAL')
    print(f'{len(names)} translation units, {len(names) - bad} identical, {bad} different')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
