#!/usr/bin/env python3
"""Generate the MoSR / MoSRv2 golden fixtures (tests/golden/mosr_*.npz, mosrv2_*.npz) by running the REAL reference.

Imports tools/gen_golden.py for its import shims and applies the same no-pin shim to MoSRv2's own DySample (mosrv2/arch.py asks for
``pin_memory=True``).  Writes only files with the two prefixes above.  Each fixture records the synthetic checkpoint's arguments, the seed,
the metadata the reference's loader inferred and the uid of the reference architecture that claimed the state dict.  The x1 MoSRv2 with
``unshuffle_mod`` has no fixture: the reference loads it wrongly (archs/mosrv2/__init__.py in this package).

Usage:  python tools/gen_golden_mosr.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth

import resselt.archs.mosrv2.arch as _v2  # noqa: E402

_v2.torch = G._TorchNoPin()  # MoSRv2's own DySample: the same shim

MOSR = [  # name, synth kwargs, input shape, seed
    ('mosr_x4_ps_d32_b2_12x14', dict(upscale=4, n_block=2, dim=32), (1, 3, 12, 14), 301),
    ('mosr_x2_ps_d40_b2_15x17', dict(upscale=2, n_block=2, dim=40), (1, 3, 15, 17), 302),
    ('mosr_x3_gps_d32_b1_13x11', dict(upscale=3, n_block=1, dim=32, upsampler='gps'), (1, 3, 13, 11), 303),
    ('mosr_x2_dys_d48_cr05_k5_b2_b2_12x16', dict(upscale=2, n_block=2, dim=48, upsampler='dys', conv_ratio=0.5, kernel_size=5), (2, 3, 12, 16), 304),
    ('mosr_x1_ps_d32_k9_b1_17x9', dict(upscale=1, n_block=1, dim=32, kernel_size=9), (1, 3, 17, 9), 305),
    ('mosr_x4_dys_d32_k3_b1_10x12', dict(upscale=4, n_block=1, dim=32, upsampler='dys', kernel_size=3, expansion_ratio=2.0), (1, 3, 10, 12), 306),
    ('mosr_x4_full_d64_b24_8x8', dict(upscale=4, n_block=24, dim=64), (1, 3, 8, 8), 307),
]
MOSRV2 = [
    ('mosrv2_x2_psd_unsh_d40_b2_13x15', dict(scale=2, n_block=2, dim=40), (1, 3, 13, 15), 311),
    ('mosrv2_x4_psd_d32_rms_b1_12x10', dict(scale=4, n_block=1, dim=32, rms_norm=True), (1, 3, 12, 10), 312),
    ('mosrv2_x1_conv_d32_b1_11x13', dict(scale=1, n_block=1, dim=32, upsampler='conv', unshuffle_mod=False), (1, 3, 11, 13), 313),
    ('mosrv2_x2_ps_d48_b2_b2_10x12', dict(scale=2, n_block=2, dim=48, upsampler='pixelshuffle', unshuffle_mod=False, mid_dim=32), (2, 3, 10, 12), 314),
    ('mosrv2_x3_ps_d32_b1_9x11', dict(scale=3, n_block=1, dim=32, upsampler='pixelshuffle', mid_dim=16), (1, 3, 9, 11), 315),
    ('mosrv2_x4_nc_d32_rms_b1_9x8', dict(scale=4, n_block=1, dim=32, upsampler='nearest+conv', rms_norm=True), (1, 3, 9, 8), 316),
    ('mosrv2_x3_nc_d32_b1_10x9', dict(scale=3, n_block=1, dim=32, upsampler='nearest+conv'), (1, 3, 10, 9), 317),
    ('mosrv2_x2_nc_unsh_d32_b1_11x9', dict(scale=2, n_block=1, dim=32, upsampler='nearest+conv'), (1, 3, 11, 9), 318),
    ('mosrv2_x2_dys_mid_d32_b1_12x13', dict(scale=2, n_block=1, dim=32, upsampler='dysample', mid_dim=16, unshuffle_mod=False), (1, 3, 12, 13), 319),
    ('mosrv2_x2_dys_unsh_d32_b1_b2_9x10', dict(scale=2, n_block=1, dim=32, upsampler='dysample', mid_dim=16), (2, 3, 9, 10), 320),
    ('mosrv2_x2_full_d64_b24_9x11', dict(scale=2, n_block=24, dim=64), (1, 3, 9, 11), 321),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_mosr.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: x {tuple(arrays["x"].shape)} -> y {tuple(arrays["y"].shape)}')


def main():
    for cases, make, arch in ((MOSR, synth.mosr_state_dict, 'mosr'), (MOSRV2, synth.mosrv2_state_dict, 'mosrv2')):
        for name, kw, shape, seed in cases:
            assert name.startswith(arch + '_')
            sd = make(seed=seed, **kw)
            model = resselt.load_from_state_dict(dict(sd)).eval()
            x = synth.synth_input(shape, seed)
            y = model(x.clone())
            save(name, dict(arch=arch, synth=kw, seed=seed, metadata=G.meta_of(model), claimed_by=claimed_by(sd)), x=x, y=y)


if __name__ == '__main__':
    main()
