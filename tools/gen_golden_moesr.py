#!/usr/bin/env python3
"""Generate the MoESR golden fixtures (tests/golden/moesr_*.npz) by running the REAL reference on the CPU.

Imports tools/gen_golden.py for its import shims (the ``dysample`` head is the shared DySample, whose ``pin_memory=True`` that module
already shims).  Writes only files with the prefix above.  Each fixture records the synthetic checkpoint's arguments, the seed, the metadata
the reference's loader inferred, the hyper-parameters it handed to the module (captured at the call), the uid of every reference
architecture that claims the state dict (``claimed_by`` the first, ``claims`` all), the names, shapes and dtypes of the reference module's
state_dict -- no weights -- and ``f64_dev``, the reference's own f32-against-f64 deviation on the case, with ``y_absmax`` to read it against.
The file round trip through the reference's own loader (``.pth``) is part of every case.

Usage:  python tools/gen_golden_moesr.py
"""

from __future__ import annotations

import copy
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth

import resselt.archs.moesr as _pkg  # noqa: E402

CASES = [  # name, synth kwargs, input shape, seed
    ('moesr_x2_psd_d32_g2b1_9x11', dict(scale=2, dim=32, n_blocks=2, n_block=1), (1, 3, 9, 11), 1101),
    ('moesr_x3_ps_d40_g1b2_e15_m20_n2_12x13', dict(scale=3, dim=40, n_blocks=1, n_block=2, expansion_factor=1.5, expansion_msg=2.0, upsampler='pixelshuffle',
                                                    upsample_dim=16), (2, 3, 12, 13), 1102),
    ('moesr_x4_nc_d48_g1b1_10x12', dict(scale=4, dim=48, n_blocks=1, n_block=1, upsampler='nearest+conv'), (1, 3, 10, 12), 1103),
    ('moesr_x2_dys_d32_g1b1_11x8', dict(scale=2, dim=32, n_blocks=1, n_block=1, upsampler='dysample'), (1, 3, 11, 8), 1104),
    ('moesr_x1_conv_d32_g1b1_13x15', dict(scale=1, dim=32, n_blocks=1, n_block=1, upsampler='conv'), (1, 3, 13, 15), 1105),
    ('moesr_x4_full_d64_g9b4_9x11', dict(scale=4, dim=64), (1, 3, 9, 11), 1106),
    ('moesr_x2_psd_d32_gray_g1b1_8x9', dict(scale=2, dim=32, n_blocks=1, n_block=1, in_ch=1, out_ch=1), (1, 1, 8, 9), 1107),
]  # fmt: skip

_captured: dict = {}
# the registered loader's own globals (the registry imports the architecture packages by walking the file system, so the module object
# it holds need not be the one ``import`` returns)
_loader_globals = resselt.archs.internal_registry.get('MoESR').load.__func__.__globals__
_RealMoESR = _loader_globals['MoESR']


def _capture(**kw):
    _captured.clear()
    _captured.update(kw)
    return _RealMoESR(**kw)


_loader_globals['MoESR'] = _pkg.MoESR = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.moesr_state_dict(seed=seed, **kw)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'moesr.pth')
            torch.save(dict(sd), path)
            model = resselt.load_from_file(path).eval()
        hyper = {k: (v if isinstance(v, (str, float)) else int(v)) for k, v in _captured.items()}
        ref_sd = model.state_dict()
        assert list(ref_sd) == list(sd) and all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype for k, v in sd.items()), name
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double()(x.double())
        who = claims(sd)
        meta = dict(arch='moesr', synth=kw, seed=seed, metadata=G.meta_of(model), hyper=hyper, claimed_by=who[0] if who else '', claims=who,
                    state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()),
                    torch=torch.__version__, generator='tools/gen_golden_moesr.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")


if __name__ == '__main__':
    main()
