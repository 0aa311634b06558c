#!/usr/bin/env python3
"""Generate the EIMN golden fixtures (tests/golden/eimn_*.npz) by running the REAL reference in eval mode.

Imports tools/gen_golden.py for its import shims.  Writes only files with the prefix above.  Each fixture records the synthetic
checkpoint's arguments, the seed, the metadata the reference's loader inferred, the uid of the reference architecture that claimed the
state dict, the hyper-parameters of the module it built and the names and shapes of that module's state_dict -- no weights.  The reference
returns its module in training mode (BatchNorm would use batch statistics): the fixtures are the ``.eval()`` forward.  Outputs larger than
48 x 48 are cropped to their top-left 48 x 48.

Usage:  python tools/gen_golden_eimn.py
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

CASES = [  # name, synth kwargs, input shape, seed
    ('eimn_x2_c64_s2_9x11', dict(embed_dims=64, scale=2, num_stages=2), (1, 3, 9, 11), 801),
    ('eimn_x4_c64_s3_5x7', dict(embed_dims=64, scale=4, num_stages=3), (1, 3, 5, 7), 802),  # the map is smaller than every halo
    ('eimn_x3_c48_s2_13x10', dict(embed_dims=48, scale=3, num_stages=2), (1, 3, 13, 10), 803),  # groups 18 / 6 / 24, hidden 127
    ('eimn_x2_c64_s2_d2_b2_20x33', dict(embed_dims=64, scale=2, num_stages=2, depths=2), (2, 3, 20, 33), 804),  # crosses tile boundaries both ways
    ('eimn_x2_c64_h128_s2_12x14', dict(embed_dims=64, scale=2, num_stages=2, hidden=128), (1, 3, 12, 14), 805),  # mlp ratio 2.0
    ('eimn_x2_c64_s16_12x12', dict(embed_dims=64, scale=2, num_stages=16), (1, 3, 12, 12), 806),  # the reference's default depth
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_eimn.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()))


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.eimn_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd))
        assert model.training  # what the loader hands out; inference callers switch to eval
        model = model.eval()
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}
        blk = model.block1[0]
        hyper = dict(num_stages=model.num_stages, depths=len(model.block1), embed_dims=model.head[0].out_channels, hidden=blk.mlp.linear_out.in_channels,
                     splits=[blk.attn.split_c1, blk.attn.split_c2, blk.attn.split_c3], reduce_channels=blk.mlp.DFFM.local_reduce.out_channels)  # fmt: skip
        meta = dict(arch='eimn', synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval', state_dict=keys, hyper=hyper)
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
        full = list(y.shape)
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y = y[:, :, :CROP, :CROP]
        save(name, dict(meta, crop=crop, y_shape=full), x=x, y=y)


if __name__ == '__main__':
    main()
