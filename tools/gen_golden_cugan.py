#!/usr/bin/env python3
"""Generate the Real-CUGAN golden fixtures (tests/golden/cugan_*.npz) by running the REAL reference.

Imports tools/gen_golden.py for its import shims and writes only files with the prefix above; no other fixture is touched.  Each fixture
records the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred and the uid of the reference
architecture that claimed the state dict.

Usage:  python tools/gen_golden_cugan.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth

CASES = [  # name, synth kwargs, input shape, seed
    ('cugan_x2_23x22', dict(variant='2x'), (1, 3, 23, 22), 301),
    ('cugan_x2_pro_b2_20x24', dict(variant='2x', pro=True), (2, 3, 20, 24), 302),
    ('cugan_x3_18x18', dict(variant='3x'), (1, 3, 18, 18), 303),
    ('cugan_x3_pro_21x26', dict(variant='3x', pro=True), (1, 3, 21, 26), 304),
    ('cugan_x4_21x25', dict(variant='4x'), (1, 3, 21, 25), 305),
    ('cugan_x4_pro_b2_20x24', dict(variant='4x', pro=True), (2, 3, 20, 24), 306),
    ('cugan_x2fast_40x44', dict(variant='2x_fast'), (1, 3, 40, 44), 307),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_cugan.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: x {tuple(arrays["x"].shape)} -> y {tuple(arrays["y"].shape)}')


def main():
    for name, kw, shape, seed in CASES:
        assert name.startswith('cugan_')
        sd = synth.cugan_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd)).eval()
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
        save(name, dict(arch='cugan', synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd)), x=x, y=y)


if __name__ == '__main__':
    main()
