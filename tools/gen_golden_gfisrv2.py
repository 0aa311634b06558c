#!/usr/bin/env python3
"""Generate the GFISRv2 golden fixtures (tests/golden/gfisrv2_*.npz) by running the REAL reference on the CPU.

Imports tools/gen_golden.py for its import shims; GFISRv2's private DySample also calls ``torch.tensor(..., pin_memory=True)``
(gfisrv2/arch.py:84-86), so the same no-pin shim is installed on that module.  Writes only files with the prefix above.  Each fixture records
the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred, the hyper-parameters it handed to the module
(captured at the call), the uid of every reference architecture that claims the state dict (``claimed_by`` the first, ``claims`` all), the
names, shapes and dtypes of the reference module's state_dict -- no weights -- and ``f64_dev``, the deviation of the reference's own f32
forward from its forward on a ``.double()`` copy (whose FourierUnit still transforms in f32, as the module is written), with ``y_absmax``
to read it against.  The file round trip through the reference's own loader (``.pth``) is part of every case.

``gfisrv2_tiny_probe.npz`` holds only the probe of the tiny inputs 1x1, 1x2, 2x1, 1x3 and 3x1: which of them make the reference raise
(and what), and input and output of those that run.

Usage:  python tools/gen_golden_gfisrv2.py
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

import resselt.archs.gfisrv2 as _pkg  # noqa: E402

B5 = dict(n_blocks=5)
CASES = [  # name, synth kwargs, input shape, seed
    ('gfisrv2_x4_psd_d48_b24_9x11', dict(), (1, 3, 9, 11), 1301),  # the default depth; odd x odd
    ('gfisrv2_x2_psd_d16_b5_b2_6x8', dict(B5, dim=16, scale=2), (2, 3, 6, 8), 1302),  # all four rotations and one wrap; even x even; batch 2
    ('gfisrv2_x3_ps_d24_m16_b5_7x10', dict(B5, dim=24, scale=3, upsampler='pixelshuffle', mid_dim=16), (1, 3, 7, 10), 1303),  # odd x even
    ('gfisrv2_x4_nc_d64_b2_8x5', dict(dim=64, n_blocks=2, scale=4, upsampler='nearest+conv'), (1, 3, 8, 5), 1304),
    ('gfisrv2_x2_dys_d16_m16_b2_5x7', dict(dim=16, n_blocks=2, scale=2, upsampler='dysample', mid_dim=16), (1, 3, 5, 7), 1305),
    ('gfisrv2_x3_dys_d24_m32_b1_6x5', dict(dim=24, n_blocks=1, scale=3, upsampler='dysample', mid_dim=32), (1, 3, 6, 5), 1306),
    ('gfisrv2_x1_conv_d16_gray_b4_11x13', dict(dim=16, n_blocks=4, scale=1, upsampler='conv', in_nc=1, out_nc=1), (1, 1, 11, 13), 1307),
    ('gfisrv2_x2_ps_d48_m24_e15_b2_4x6', dict(dim=48, n_blocks=2, scale=2, upsampler='pixelshuffle', mid_dim=24, expansion_ratio=1.5), (1, 3, 4, 6), 1308),
    ('gfisrv2_x3_nc_d16_b1_b2_5x4', dict(dim=16, n_blocks=1, scale=3, upsampler='nearest+conv'), (2, 3, 5, 4), 1309),
]  # fmt: skip
PROBE = ('gfisrv2_tiny_probe', dict(dim=16, n_blocks=1, scale=2), ((1, 1), (1, 2), (2, 1), (1, 3), (3, 1)), 1320)

_captured: dict = {}
# the registered loader's own globals (the registry imports the architecture packages by walking the file system, so the module object
# it holds need not be the one ``import`` returns)
_loader_globals = resselt.archs.internal_registry.get('GFISRV2').load.__func__.__globals__
_RealGFISRV2 = _loader_globals['GFISRV2']
sys.modules[_RealGFISRV2.__module__].torch = G._TorchNoPin()


def _capture(**kw):
    _captured.clear()
    _captured.update(kw)
    return _RealGFISRV2(**kw)


_loader_globals['GFISRV2'] = _pkg.GFISRV2 = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def load(sd):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'gfisrv2.pth')
        torch.save(dict(sd), path)
        return resselt.load_from_file(path).eval()


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.gfisrv2_state_dict(seed=seed, **kw)
        model = load(sd)
        hyper = {k: (v if isinstance(v, (str, float, bool)) else int(v)) for k, v in _captured.items()}
        ref_sd = model.state_dict()
        assert list(ref_sd) == list(sd) and all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype for k, v in sd.items()), name
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double()(x.double())
        who = claims(sd)
        meta = dict(arch='gfisrv2', synth=kw, seed=seed, metadata=G.meta_of(model), hyper=hyper, claimed_by=who[0] if who else '', claims=who,
                    state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()),
                    torch=torch.__version__, generator='tools/gen_golden_gfisrv2.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        assert size <= 64 * 1024, (name, size)
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")

    name, kw, sizes, seed = PROBE
    model = load(synth.gfisrv2_state_dict(seed=seed, **kw))
    results, arrays = [], {}
    for h, w in sizes:
        x = synth.synth_input((1, 3, h, w), seed)
        try:
            with torch.no_grad():
                y = model(x.clone())
            results.append(dict(size=[h, w], raises=None))
            arrays[f'x_{h}x{w}'], arrays[f'y_{h}x{w}'] = x.numpy(), y.numpy()
        except Exception as e:  # noqa: BLE001  (the probe records whatever the reference raises)
            results.append(dict(size=[h, w], raises=type(e).__name__, message=str(e).splitlines()[0][:160]))
    meta = dict(arch='gfisrv2', synth=kw, seed=seed, probe=results, torch=torch.__version__, generator='tools/gen_golden_gfisrv2.py')
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **arrays)
    print(name, results)


if __name__ == '__main__':
    main()
