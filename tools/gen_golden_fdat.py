#!/usr/bin/env python3
"""Generate the FDAT golden fixtures (tests/golden/fdat_*.npz) by running the REAL reference in eval mode.

Imports tools/gen_golden.py for its import shims; FDAT's private DySample also calls ``torch.tensor(..., pin_memory=True)``
(fdat/arch.py:90), so the same no-pin shim is installed on that module.  Writes only files with the prefix above.  Each fixture records the
synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred and the uid of the reference architecture that
claimed the state dict, and the names and shapes of the reference module's state_dict -- no weights.  Outputs larger than 48 x 48 are cropped to their top-left 48 x 48.

Usage:  python tools/gen_golden_fdat.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

import resselt.archs.fdat.arch as _ref_fdat  # noqa: E402

_ref_fdat.torch = G._TorchNoPin()
torch, resselt, synth = G.torch, G.resselt, G.synth
CROP = 48

B = dict(embed_dim=48, num_groups=1, depth_per_group=1, num_heads=4, window_size=4, mid_dim=32)
CASES = [  # name, synth kwargs, input shape, seed
    ('fdat_x2_tconv_e48_w4_13x10', dict(B, scale=2, upsampler_type='transpose+conv'), (1, 3, 13, 10), 501),
    ('fdat_x3_tconv_e48_w4_9x11', dict(B, scale=3, upsampler_type='transpose+conv'), (1, 3, 9, 11), 502),
    ('fdat_x4_tconv_e48_w8_g2_10x9', dict(B, scale=4, window_size=8, num_groups=2, upsampler_type='transpose+conv'), (1, 3, 10, 9), 503),
    ('fdat_x1_conv_e48_w4_12x7', dict(B, scale=1, upsampler_type='conv'), (1, 3, 12, 7), 504),
    ('fdat_x2_conv_e48_w4_3x5', dict(B, scale=2, upsampler_type='conv'), (1, 3, 3, 5), 505),
    ('fdat_x3_psd_e48_w4_10x8', dict(B, scale=3, upsampler_type='pixelshuffledirect'), (1, 3, 10, 8), 506),
    ('fdat_x4_ps_e48_w4_9x8', dict(B, scale=4, upsampler_type='pixelshuffle'), (1, 3, 9, 8), 507),
    ('fdat_x3_nc_e48_w4_8x9', dict(B, scale=3, upsampler_type='nearest+conv'), (1, 3, 8, 9), 508),
    ('fdat_x2_nc_e48_w4_b2_9x10', dict(B, scale=2, upsampler_type='nearest+conv'), (2, 3, 9, 10), 509),
    ('fdat_x2_dys_e48_w4_10x9', dict(B, scale=2, upsampler_type='dysample'), (1, 3, 10, 9), 510),
    ('fdat_x4_dys_mid48_e48_w4_8x8', dict(B, scale=4, mid_dim=48, upsampler_type='dysample'), (1, 3, 8, 8), 511),
    ('fdat_x2_lda_e48_w4_11x9', dict(B, scale=2, upsampler_type='lda'), (1, 3, 11, 9), 512),
    ('fdat_x3_lda_e48_w4_9x10', dict(B, scale=3, upsampler_type='lda'), (1, 3, 9, 10), 513),
    ('fdat_x4_lda_mid48_e48_w4_8x9', dict(B, scale=4, mid_dim=48, upsampler_type='lda'), (1, 3, 8, 9), 514),
    ('fdat_x2_pa_e48_w4_10x11', dict(B, scale=2, upsampler_type='pa_up'), (1, 3, 10, 11), 515),
    ('fdat_x3_pa_e48_w4_9x9', dict(B, scale=3, upsampler_type='pa_up'), (1, 3, 9, 9), 516),
    ('fdat_x4_pa_e48_w4_8x10', dict(B, scale=4, upsampler_type='pa_up'), (1, 3, 8, 10), 517),
    ('fdat_x1_unsh_conv_e48_w4_13x14', dict(B, scale=1, upsampler_type='conv', unshuffle_mod=True), (1, 3, 13, 14), 518),
    ('fdat_x2_unsh_tconv_e48_w4_11x13', dict(B, scale=2, upsampler_type='transpose+conv', unshuffle_mod=True), (1, 3, 11, 13), 519),
    ('fdat_x2_tconv_e64_w16_hd16_ffn15_20x18', dict(B, scale=2, embed_dim=64, window_size=16, ffn_expansion_ratio=1.5, upsampler_type='transpose+conv'),
     (1, 3, 20, 18), 520),  # fmt: skip
    ('fdat_x2_tconv_gray_e48_w4_b2_9x7', dict(B, num_in_ch=1, num_out_ch=1, scale=2, upsampler_type='transpose+conv'), (2, 1, 9, 7), 521),
    ('fdat_x4_tconv_e180_h6_w8_9x8', dict(B, embed_dim=180, num_heads=6, window_size=8, scale=4, upsampler_type='transpose+conv'), (1, 3, 9, 8), 523),
    ('fdat_x4_tconv_default_12x10', dict(embed_dim=120, num_groups=4, depth_per_group=3, num_heads=4, window_size=8, mid_dim=64, scale=4), (1, 3, 12, 10),
     522),  # fmt: skip
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_fdat.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: ' + ', '.join(f'{k} {tuple(np.asarray(v).shape)}' for k, v in arrays.items()))


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.fdat_state_dict(seed=seed, **kw)
        model = resselt.load_from_state_dict(dict(sd)).eval()
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}  # the reference module's state_dict: names and shapes
        meta = dict(arch='fdat', synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd), mode='eval', state_dict=keys)
        x = synth.synth_input(shape, seed)
        y = model(x.clone())
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y = y[:, :, :CROP, :CROP]
        save(name, dict(meta, crop=crop, y_shape=list(model(x.clone()).shape) if crop else list(y.shape)), x=x, y=y)


if __name__ == '__main__':
    main()
