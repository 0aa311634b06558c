#!/usr/bin/env python3
"""Generate the RCAN golden fixtures (tests/golden/rcan_*.npz) by running the REAL reference in eval mode.

Imports tools/gen_golden.py for its import shims.  Writes only files with the prefix above.  Each fixture records the synthetic
checkpoint's arguments, the seed, the metadata the reference's loader inferred and the uid of the reference architecture that claimed the
state dict, and the names and shapes of the reference module's state_dict -- no weights.  The reference multiplies its input by rgb_range
IN PLACE, so the model is given a clone and the fixture keeps the caller's values.  Outputs larger than 48 x 48 are cropped to their
top-left 48 x 48.

Usage:  python tools/gen_golden_rcan.py
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

B = dict(n_resgroups=1, n_resblocks=2, n_feats=64, reduction=16, norm=True)
CASES = [  # name, synth kwargs, input shape, seed
    ('rcan_x2_c64_g1b2_19x21', dict(B, scale=2), (1, 3, 19, 21), 701),
    ('rcan_x3_c64_g1b2_nonorm_14x17', dict(B, scale=3, norm=False), (1, 3, 14, 17), 702),
    ('rcan_x4_c64_g2b3_13x15', dict(B, scale=4, n_resgroups=2, n_resblocks=3), (1, 3, 13, 15), 703),
    ('rcan_x8_c64_g1b1_9x11', dict(B, scale=8, n_resblocks=1), (1, 3, 9, 11), 704),
    ('rcan_x2_unshuffle_c64_g1b2_21x19', dict(B, scale=2, unshuffle_mod=True), (1, 3, 21, 19), 705),
    ('rcan_x1_unshuffle_c64_g1b2_nonorm_22x27', dict(B, scale=1, unshuffle_mod=True, norm=False), (1, 3, 22, 27), 706),
    ('rcan_x2_gray_c64_g1b2_b2_15x14', dict(B, scale=2, n_colors=1, norm=False), (2, 1, 15, 14), 707),
    ('rcan_x2_c48_r8_g1b2_17x18', dict(B, scale=2, n_feats=48, reduction=8), (1, 3, 17, 18), 708),
    ('rcan_x4_c32_r4_g1b1_nonorm_12x13', dict(B, scale=4, n_feats=32, reduction=4, n_resblocks=1, norm=False), (1, 3, 12, 13), 709),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_rcan.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()))


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.rcan_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd)).eval()
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}  # the reference module's state_dict: names and shapes
        hyper = dict(downscale_factor=model.downscale_factor, scale=model.scale, rgb_range=model.rgb_range)
        meta = dict(arch='rcan', synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval', state_dict=keys, hyper=hyper)
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())  # forward multiplies its argument in place (arch.py:323)
        full = list(y.shape)
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y = y[:, :, :CROP, :CROP]
        save(name, dict(meta, crop=crop, y_shape=full), x=x, y=y)


if __name__ == '__main__':
    main()
