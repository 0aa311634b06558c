#!/usr/bin/env python3
"""Generate the RHA golden fixtures (tests/golden/rha_*.npz) by running the REAL reference in eval mode on the CPU.

Imports tools/gen_golden.py for its import shims and applies the same no-pin shim to RHA's own DySample (rha/arch.py asks for
``pin_memory=True``).  Writes only files with the prefix above.  Each fixture records the synthetic checkpoint's arguments, the seed, the
metadata and hyper-parameters the reference's loader inferred, the uid of the reference architecture that claimed the state dict, and the
names and shapes of the reference module's state_dict -- no weights.  Outputs larger than 48 x 48 are cropped to their top-left 48 x 48.
``f64_dev`` is the reference's own f32-against-f64 deviation on the case, ``y_absmax`` the scale it is to be read against.

Usage:  python tools/gen_golden_rha.py
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

import resselt.archs.rha.arch as _rha  # noqa: E402

_rha.torch = G._TorchNoPin()  # RHA's own DySample: the same shim
CROP = 48

CASES = [  # name, synth kwargs, input shape, seed
    ('rha_x2_psd_d32_dn21_g2b2_13x18', dict(dim=32, scale=2, down_list=(2, 1), group_blocks=2, res_blocks=2, window_size=8), (1, 3, 13, 18), 901),
    ('rha_x4_ps_d64_dn84_g2b2_40x70', dict(dim=64, scale=4, down_list=(8, 4), group_blocks=2, res_blocks=2, window_size=8, upsample='pixelshuffle', mid_dim=32),
     (1, 3, 40, 70), 902),
    ('rha_x3_dys_d48_dn2_g1b3_w4_n2_9x11', dict(dim=48, scale=3, down_list=(2,), group_blocks=1, res_blocks=3, window_size=4, upsample='dysample', mid_dim=32),
     (2, 3, 9, 11), 903),
    # pooled 16 x 8 with window 8: one window column, so the shifted window wraps onto itself
    ('rha_x1_conv_d32_gray_dn4_g1b2_33x20', dict(dim=32, scale=1, in_ch=1, out_ch=1, down_list=(4,), group_blocks=1, res_blocks=2, window_size=8, upsample='conv'),
     (1, 1, 33, 20), 904),
    ('rha_x2_nc_d32_e20_dn2_g1b2_w4_10x12', dict(dim=32, scale=2, down_list=(2,), expansion_ratio=2.0, group_blocks=1, res_blocks=2, window_size=4,
                                                 upsample='nearest+conv'), (1, 3, 10, 12), 905),
    ('rha_x2_psd_d16_e10_dn1_g1b2_w4_7x9', dict(dim=16, scale=2, down_list=(1,), expansion_ratio=1.0, group_blocks=1, res_blocks=2, window_size=4),
     (1, 3, 7, 9), 906),  # hidden == dim: no i channels
]  # fmt: skip


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_rha.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()) + f"  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}")


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.rha_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd)).eval()
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}  # the reference module's state_dict: names and shapes
        blk = model.body[0].body[0]
        hyper = dict(dim=model.to_feat.out_channels, in_ch=model.to_feat.in_channels, group_blocks=len(model.body), res_blocks=len(model.body[0].body) - 2,
                     down_list=[int(g.down_sample) for g in model.body], hidden=blk.fc2.in_channels, window_size=blk.conv.att[2].window_size,
                     head=_rha.SampleMods.__args__[int(model.to_img.MetaUpsample[1])], scale=model.scale, out_ch=int(model.to_img.MetaUpsample[4]),
                     mid_dim=int(model.to_img.MetaUpsample[5]), pad=int(model.pad))  # fmt: skip
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double()(x.double())
        meta = dict(arch='rha', synth=dict(kw, down_list=list(kw['down_list'])), seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval',
                    state_dict=keys, hyper=hyper, y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()))
        full = list(y.shape)
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y = y[:, :, :CROP, :CROP]
        save(name, dict(meta, crop=crop, y_shape=full), x=x, y=y)


if __name__ == '__main__':
    main()
