#!/usr/bin/env python3
"""Register / scratch / LDS usage of every gfx950 kernel in a built libresselt_amd.so, and the comparison of two builds.

    python tools/kernel_resources.py LIB                 one CSV line per kernel symbol
    python tools/kernel_resources.py BEFORE.so AFTER.so  kernels whose numbers differ, kernels only in one build; exit status 1 if any
                                                         kernel of BEFORE is missing from AFTER or changed

The numbers are the code objects' own metadata (`llvm-readelf --notes`: .vgpr_count, .agpr_count, .sgpr_count,
.private_segment_fixed_size = scratch bytes, .group_segment_fixed_size = LDS bytes).  The device code objects are cut out of the
library's .hip_fatbin section (uncompressed clang offload bundles, one per translation unit).
"""

from __future__ import annotations

import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')


def code_objects(lib: str) -> list[bytes]:
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fat.bin')
        subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', f'.hip_fatbin={fat}', lib, os.path.join(tmp, 'copy.so')], check=True)
        blob = open(fat, 'rb').read()
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from('<Q', blob, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', blob, q)
            triple = blob[q + 24 : q + 24 + tl].decode()
            q += 24 + tl
            if 'amdgcn' in triple and size:
                out.append(blob[pos + off : pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    if not out:
        raise SystemExit(f'{lib}: no device code objects found (compressed bundles are not handled)')
    return out


def kernels(lib: str) -> dict:
    res = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix='.co') as fh:
            fh.write(co)
            fh.flush()
            notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', fh.name], check=True, capture_output=True, text=True).stdout
        for block in re.split(r'\n\s*- \.agpr_count:', notes)[1:]:
            block = '.agpr_count:' + block
            name = re.search(r'\.name:\s+(\S+)', block).group(1)
            res[name] = tuple(int(re.search(rf'\.{f}:\s+(\d+)', block).group(1)) for f in FIELDS)
    return res


def main(argv):
    if len(argv) == 1:
        print('kernel,' + ','.join(FIELDS))
        for name, v in sorted(kernels(argv[0]).items()):
            print(name + ',' + ','.join(map(str, v)))
        return 0
    a, b = kernels(argv[0]), kernels(argv[1])
    changed = {k for k in a if k in b and a[k] != b[k]}
    missing = sorted(set(a) - set(b))
    print(f'{len(a)} kernels before, {len(b)} after, {len(set(b) - set(a))} new, {len(missing)} missing, {len(changed)} changed  ({", ".join(FIELDS)})')
    for k in sorted(changed):
        print(f'CHANGED {k}: {a[k]} -> {b[k]}')
    for k in missing:
        print(f'MISSING {k}')
    for k in sorted(set(b) - set(a)):
        print(f'NEW {k}: {b[k]}')
    return 1 if changed or missing else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
