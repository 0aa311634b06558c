#!/usr/bin/env python3
"""Generate the OmniSR golden fixtures (tests/golden/omnisr_*.npz) by running the REAL reference in eval mode.

Imports tools/gen_golden.py for its import shims.  Writes only files with the prefix above.  Each fixture records the synthetic
checkpoint's arguments, the seed, the metadata the reference's loader inferred and the uid of the reference architecture that claimed the
state dict, and the names and shapes of the reference module's state_dict -- no weights.  Outputs larger than 48 x 48 are cropped to their
top-left 48 x 48.

Usage:  python tools/gen_golden_omnisr.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth
CROP = 48

B = dict(num_feat=32, res_num=1, block_num=1, pe=True, window_size=4, bias=True)
CASES = [  # name, synth kwargs, input shape, seed
    ('omnisr_x1_c32_w4_16x14', dict(B, up_scale=1), (1, 3, 16, 14), 601),
    ('omnisr_x2_c32_w4_25x17', dict(B, up_scale=2), (1, 3, 25, 17), 602),
    ('omnisr_x3_c32_w8_nope_15x18', dict(B, up_scale=3, pe=False, window_size=8), (1, 3, 15, 18), 603),
    ('omnisr_x4_c32_w4_nobias_13x16', dict(B, up_scale=4, bias=False), (1, 3, 13, 16), 604),
    ('omnisr_x2_c48_w8_20x17', dict(B, num_feat=48, window_size=8, up_scale=2), (1, 3, 20, 17), 605),
    ('omnisr_x2_c64_w8_r2_b2_16x19', dict(B, num_feat=64, window_size=8, res_num=2, block_num=2, up_scale=2), (1, 3, 16, 19), 606),
    ('omnisr_x2_c32_w4_b2_gray_14x15', dict(B, num_in_ch=1, up_scale=2), (2, 1, 14, 15), 607),
    ('omnisr_x2_c44_w8_nope_nobias_17x13', dict(B, num_feat=44, up_scale=2, pe=False, bias=False, window_size=8), (1, 3, 17, 13), 608),
    ('omnisr_x4_default_17x23', dict(num_feat=64, res_num=5, block_num=1, pe=True, window_size=8, up_scale=4, bias=True), (1, 3, 17, 23), 609),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_omnisr.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()))


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.omnisr_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd)).eval()
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}  # the reference module's state_dict: names and shapes
        meta = dict(arch='omnisr', synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval', state_dict=keys)
        x = synth.synth_input(shape, seed)
        y = model(x.clone())
        full = list(y.shape)
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y = y[:, :, :CROP, :CROP]
        save(name, dict(meta, crop=crop, y_shape=full), x=x, y=y)


if __name__ == '__main__':
    main()
