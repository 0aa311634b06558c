#!/usr/bin/env python3
"""Generate the PLKSR / RealPLKSR golden fixtures (tests/golden/plksr_*.npz, realplksr_*.npz) by running the REAL reference.

Imports tools/gen_golden.py for its two import shims (typing.Self, DySample's pin_memory) and writes only files with the two prefixes
above; no other fixture is touched.  Each fixture records the synthetic checkpoint's arguments, the seed, the metadata the reference's
loader inferred and the uid of the reference architecture that claimed the state dict.

Usage:  python tools/gen_golden_plksr.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth

REAL = [  # name, synth kwargs, input shape, seed
    ('realplksr_x4_ps_d64_b2_16x20', dict(dim=64, n_blocks=2, upscale=4), (1, 3, 16, 20), 201),
    ('realplksr_x2_dys_d64_b2_20x24', dict(dim=64, n_blocks=2, upscale=2, dysample=True), (1, 3, 20, 24), 202),
    ('realplksr_x3_dys_d32_b2_17x19', dict(dim=32, n_blocks=2, upscale=3, dysample=True), (1, 3, 17, 19), 203),
    ('realplksr_x4_dys_d32_b1_b2_12x16', dict(dim=32, n_blocks=1, upscale=4, dysample=True), (2, 3, 12, 16), 204),
    ('realplksr_x2_ps_d96_b1_16x16', dict(dim=96, n_blocks=1, upscale=2), (1, 3, 16, 16), 205),
    ('realplksr_x2_ps_noea_d32_b2_16x16', dict(dim=32, n_blocks=2, upscale=2, use_ea=False), (1, 3, 16, 16), 206),
    ('realplksr_x2_ps_d32_b2_17x23', dict(dim=32, n_blocks=2, upscale=2), (1, 3, 17, 23), 207),
    ('realplksr_x1_dys_d32_b2_64x64', dict(dim=32, n_blocks=2, upscale=1, dysample=True), (1, 3, 64, 64), 208),
    ('realplksr_x2_ps_k9_d32_b4_20x20', dict(dim=32, n_blocks=4, upscale=2, kernel_size=9), (1, 3, 20, 20), 209),
]
PLK = [
    ('plksr_x2_dccm_d32_b2_16x20', dict(dim=32, n_blocks=2, upscale=2, ccm_type='DCCM'), (1, 3, 16, 20), 211),
    ('plksr_x2_ccm_d32_b2_15x17', dict(dim=32, n_blocks=2, upscale=2, ccm_type='CCM'), (1, 3, 15, 17), 212),
    ('plksr_x2_iccm_noea_d32_b2_16x16', dict(dim=32, n_blocks=2, upscale=2, ccm_type='ICCM', use_ea=False), (1, 3, 16, 16), 213),
    ('plksr_x2_rect_d32_b2_16x16', dict(dim=32, n_blocks=2, upscale=2, lk_type='RectSparsePLK'), (1, 3, 16, 16), 214),
    ('plksr_x2_sparse_d32_b2_16x16', dict(dim=32, n_blocks=2, upscale=2, lk_type='SparsePLK'), (1, 3, 16, 16), 215),
    ('plksr_x3_dccm_d64_b2_13x17', dict(dim=64, n_blocks=2, upscale=3), (1, 3, 13, 17), 216),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_plksr.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: x {tuple(arrays["x"].shape)} -> y {tuple(arrays["y"].shape)}')


def main():
    for cases, make, arch in ((REAL, synth.realplksr_state_dict, 'realplksr'), (PLK, synth.plksr_state_dict, 'plksr')):
        for name, kw, shape, seed in cases:
            assert name.startswith(arch + '_')
            sd = make(seed=seed, **kw)
            model = resselt.load_from_state_dict(dict(sd)).eval()
            x = synth.synth_input(shape, seed)
            y = model(x.clone())  # (PLKConv2d writes into its input in eval mode)
            save(name, dict(arch=arch, synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd)), x=x, y=y)


if __name__ == '__main__':
    main()
