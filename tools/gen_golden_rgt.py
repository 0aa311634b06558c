#!/usr/bin/env python3
"""Generate the RGT golden fixtures (tests/golden/rgt_*.npz) by running the REAL reference in eval mode.

Imports tools/gen_golden.py for its import shims.  Writes only files with the prefix above.  Each fixture records the synthetic
checkpoint's arguments, the seed, the metadata the reference's loader inferred and the uid of the reference architecture that claimed the
state dict.  The t = 3 case (64 x 1024) stores its input as 8-bit codes (x = codes / 255) and a crop of the output (rows and columns
[0, 32) of the x2 output) to stay small.

Usage:  python tools/gen_golden_rgt.py
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
    ('rgt_x2_e48_s2x4_d2_1conv_16x16', dict(embed_dim=48, depth=(2,), num_heads=(4,), split_size=(2, 4), upscale=2), (1, 3, 16, 16), 401),
    ('rgt_x4_e48_s4x8_d2_2_3conv_nobias_b2_21x18', dict(embed_dim=48, depth=(2, 2), num_heads=(4, 2), split_size=(4, 8), upscale=4, resi='3conv',
                                                        qkv_bias=False), (2, 3, 21, 18), 402),  # fmt: skip
    ('rgt_x3_e48_s8x32_d3_cr075_33x40', dict(embed_dim=48, depth=(3,), num_heads=(4,), split_size=(8, 32), upscale=3, c_ratio=0.75), (1, 3, 33, 40), 403),
    ('rgt_x2_e64_s4x4_d4_mlp4_gray_20x37', dict(in_chans=1, embed_dim=64, depth=(4,), num_heads=(4,), split_size=(4, 4), upscale=2, mlp_ratio=4.0),
     (1, 1, 20, 37), 404),  # fmt: skip
    ('rgt_x4_e36_s8x32_d6x3_rgts_17x23', dict(embed_dim=36, depth=(6, 6, 6), num_heads=(6, 6, 6), split_size=(8, 32), upscale=4), (1, 3, 17, 23), 405),
    ('rgt_x2_e180_s8x32_d2_h6_48x64', dict(embed_dim=180, depth=(2,), num_heads=(6,), split_size=(8, 32), upscale=2), (1, 3, 48, 64), 406),
]
T3 = ('rgt_x2_e32_s2x4_d2_t3_64x1024', dict(embed_dim=32, depth=(2,), num_heads=(2,), split_size=(2, 4), upscale=2), (1, 3, 64, 1024), 407)


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_rgt.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()))


def run(name, kw, seed):
    sd = synth.rgt_state_dict(seed=seed, **kw)
    model = resselt.load_from_state_dict(dict(sd)).eval()
    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    return sd, model, dict(arch='rgt', synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval')


def main():
    for name, kw, shape, seed in CASES:
        sd, model, meta = run(name, kw, seed)
        x = synth.synth_input(shape, seed)
        save(name, meta, x=x, y=model(x.clone()))
    name, kw, shape, seed = T3
    sd, model, meta = run(name, kw, seed)
    codes = (synth.synth_input(shape, seed) * 256).floor().clamp(0, 255).to(torch.uint8)
    y = model(codes.float() / 255)
    save(name, dict(meta, crop=[0, 32, 0, 32], input='u8/255'), x_u8=codes, y_crop=y[:, :, :32, :32])


if __name__ == '__main__':
    main()
