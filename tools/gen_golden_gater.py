#!/usr/bin/env python3
"""Generate the GateR golden fixtures (tests/golden/gater_*.npz) by running the REAL reference in eval mode on the CPU.

Imports tools/gen_golden.py for its import shims.  Writes only files with the prefix above.  Each fixture records the synthetic
checkpoint's arguments, the seed, the metadata and hyper-parameters the reference's loader inferred, the uid of the reference architecture
that claimed the state dict, and the names and shapes of the reference module's state_dict -- no weights.  Outputs larger than 48 x 48 are
cropped to their top-left 48 x 48.  ``f64_dev`` is the reference's own f32-against-f64 deviation on the case, ``y_absmax`` the scale it is
to be read against.

Usage:  python tools/gen_golden_gater.py
"""

from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth
CROP = 48

ONES = (1,) * 7
CASES = [  # name, synth kwargs, input shape, seed
    ('gater_d24_13x18', dict(dim=24, in_ch=3, num_blocks=ONES, latent_att=False), (1, 3, 13, 18), 801),
    ('gater_d24_att_b2_24x40', dict(dim=24, in_ch=3, num_blocks=(1, 1, 1, 2, 1, 1, 1), latent_att=True), (1, 3, 24, 40), 802),
    ('gater_d24_att_n2_13x18', dict(dim=24, in_ch=3, num_blocks=ONES, latent_att=True), (2, 3, 13, 18), 803),
    ('gater_d48_att_72x56', dict(dim=48, in_ch=3, num_blocks=ONES, latent_att=True), (1, 3, 72, 56), 804),
    ('gater_d48_21x35', dict(dim=48, in_ch=3, num_blocks=ONES, latent_att=False), (1, 3, 21, 35), 805),
    ('gater_d24_att_gray_8x8', dict(dim=24, in_ch=1, num_blocks=ONES, latent_att=True), (1, 1, 8, 8), 806),
    ('gater_d24_att_b2121212_9x9', dict(dim=24, in_ch=3, num_blocks=(2, 1, 2, 1, 2, 1, 2), latent_att=True), (1, 3, 9, 9), 807),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_gater.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()) + f"  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}")


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.gater_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd)).eval()
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}  # the reference module's state_dict: names and shapes
        lat = model.latent[1].gated[0]
        hyper = dict(dim=model.in_to_dim.out_channels, in_ch=model.in_to_dim.in_channels, latent_att=hasattr(lat.conv, 'focusing_factor'),
                     num_blocks=[len(b.gated) for b in (model.enc0, model.enc1[1], model.enc2[1], model.latent[1], model.dec0[1], model.dec1[1], model.dec2[0])])
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double()(x.double())
        meta = dict(arch='gater', synth=dict(kw, num_blocks=list(kw['num_blocks'])), seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval',
                    state_dict=keys, hyper=hyper, y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()))
        full = list(y.shape)
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y = y[:, :, :CROP, :CROP]
        save(name, dict(meta, crop=crop, y_shape=full), x=x, y=y)


if __name__ == '__main__':
    main()
