#!/usr/bin/env python3
"""Generate the FIGSR golden fixtures (tests/golden/figsr_*.npz) by running the REAL reference on the CPU.

Imports tools/gen_golden.py for its import shims; FIGSR's private DySample also calls ``torch.tensor(..., pin_memory=True)``
(figsr/arch.py:90), so the same no-pin shim is installed on that module.  Writes only files with the prefix above.  Each fixture records
the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred, the hyper-parameters it handed to the module
(captured at the call), the uid of every reference architecture that claims the state dict (``claimed_by`` the first, ``claims`` all), the
names, shapes and dtypes of the reference module's state_dict -- no weights -- and ``f64_dev``, the deviation of the reference's own f32
forward from its forward on a ``.double()`` copy (whose FourierUnit still transforms in f32, as the module is written), with ``y_absmax``
to read it against.  The file round trip through the reference's own loader (``.pth``) is part of every case.

``figsr_probe.npz`` holds only the probe of where the reference itself refuses: a one-block checkpoint (not detected), a one-channel
model (loads, raises in forward), the input sizes around the reflect pad's limit, and a checkpoint whose halves are not the
(n // 2, n - n // 2) split (the module cannot take the state dict).

Usage:  python tools/gen_golden_figsr.py
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

import resselt.archs.figsr as _pkg  # noqa: E402

B2 = dict(dim=32, n_blocks=2)
CASES = [  # name, synth kwargs, input shape, seed
    ('figsr_x4_psd_d48_b24_9x11', dict(), (1, 3, 9, 11), 1401),  # the default model; odd x odd
    ('figsr_x2_psd_d32_b2_n2_6x8', dict(B2, scale=2), (2, 3, 6, 8), 1402),  # batch 2; even x even; the smallest legal side
    ('figsr_x3_ps_d40_m16_b3_7x10', dict(dim=40, n_blocks=3, scale=3, upsampler='pixelshuffle', mid_dim=16), (1, 3, 7, 10), 1403),  # halves 1 + 2; odd x even
    ('figsr_x4_nc_d64_b2_8x7', dict(dim=64, n_blocks=2, scale=4, upsampler='nearest+conv'), (1, 3, 8, 7), 1404),  # even x odd
    ('figsr_x2_dys_d32_m16_b2_6x6', dict(B2, scale=2, upsampler='dysample', mid_dim=16), (1, 3, 6, 6), 1405),
    ('figsr_x3_dys_d32_m32_b3_7x9', dict(dim=32, n_blocks=3, scale=3, upsampler='dysample', mid_dim=32), (1, 3, 7, 9), 1406),  # DySample on the features themselves
    ('figsr_x1_conv_d32_b2_11x13', dict(B2, scale=1, upsampler='conv'), (1, 3, 11, 13), 1407),
    ('figsr_x2_psd_d64_gc16_b2_8x9', dict(dim=64, n_blocks=2, scale=2, gc=16), (1, 3, 8, 9), 1408),  # two planes per band
    ('figsr_x2_ps_d32_m24_k7_11_e2_b2_9x6', dict(B2, scale=2, upsampler='pixelshuffle', mid_dim=24, square_kernel_size=7, band_kernel_size=11, expansion_ratio=2.0,
                                                  shift=(0.4, 0.5, 0.55), scale_norm=(0.2, 0.25, 0.15)), (1, 3, 9, 6), 1409),  # hidden 64; a learned normalisation
    ('figsr_x3_nc_d32_b2_n2_6x7', dict(B2, scale=3, upsampler='nearest+conv', shift=(0.45, 0.4, 0.5), scale_norm=(0.18, 0.16, 0.2)), (2, 3, 6, 7), 1410),
    ('figsr_x4_ps_d32_m16_b2_7x6', dict(B2, scale=4, upsampler='pixelshuffle', mid_dim=16), (1, 3, 7, 6), 1411),  # two shuffle stages
]  # fmt: skip
PROBE = ('figsr_probe', dict(B2, scale=2), ((5, 5), (5, 6), (4, 8), (6, 6), (8, 9), (12, 7)), 1420)

_captured: dict = {}
# the registered loader's own globals (the registry imports the architecture packages by walking the file system, so the module object
# it holds need not be the one ``import`` returns)
_loader_globals = resselt.archs.internal_registry.get('FIGSR').load.__func__.__globals__
_RealFIGSR = _loader_globals['FIGSR']
sys.modules[_RealFIGSR.__module__].torch = G._TorchNoPin()


def _capture(**kw):
    _captured.clear()
    _captured.update(kw)
    return _RealFIGSR(**kw)


_loader_globals['FIGSR'] = _pkg.FIGSR = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def load(sd):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'figsr.pth')
        torch.save(dict(sd), path)
        return resselt.load_from_file(path).eval()


def _raises(fn) -> dict:
    try:
        fn()
        return dict(raises=None)
    except Exception as e:  # noqa: BLE001  (the probe records whatever the reference raises)
        return dict(raises=type(e).__name__, message=(str(e).splitlines() or [''])[0][:160])


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.figsr_state_dict(seed=seed, **kw)
        model = load(sd)
        hyper = {k: (v if isinstance(v, (str, float, bool)) else int(v)) for k, v in _captured.items()}
        ref_sd = model.state_dict()
        assert list(ref_sd) == list(sd) and all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype for k, v in sd.items()), name
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double()(x.double())
        who = claims(sd)
        meta = dict(arch='figsr', synth=kw, seed=seed, metadata=G.meta_of(model), hyper=hyper, claimed_by=who[0] if who else '', claims=who,
                    state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()),
                    torch=torch.__version__, generator='tools/gen_golden_figsr.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        assert size <= 64 * 1024, (name, size)
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")

    name, kw, sizes, seed = PROBE
    model = load(synth.figsr_state_dict(seed=seed, **kw))
    results, arrays = [], {}
    for h, w in sizes:
        x = synth.synth_input((1, 3, h, w), seed)
        r = _raises(lambda: arrays.__setitem__(f'y_{h}x{w}', model(x.clone()).numpy()))
        if r['raises'] is None:
            arrays[f'x_{h}x{w}'] = x.numpy()
        results.append(dict(size=[h, w], **r))
    one_block = dict(synth=dict(dim=32, n_blocks=1, scale=2), **_raises(lambda: resselt.load_from_state_dict(dict(synth.figsr_state_dict(dim=32, n_blocks=1, scale=2, seed=seed)))))
    gray_kw = dict(B2, scale=2, in_nc=1, out_nc=1)
    gray = dict(synth=gray_kw, load=_raises(lambda: load(synth.figsr_state_dict(seed=seed, **gray_kw))))
    if gray['load']['raises'] is None:
        gm = load(synth.figsr_state_dict(seed=seed, **gray_kw))
        gray['forward'] = _raises(lambda: gm(synth.synth_input((1, 1, 8, 8), seed)))
        gray['metadata'] = G.meta_of(gm)
    uneven_kw = dict(dim=32, n_blocks=4, scale=2, halves=[1, 3])
    uneven = dict(synth=uneven_kw, **_raises(lambda: resselt.load_from_state_dict(dict(synth.figsr_state_dict(seed=seed, **uneven_kw)))))
    meta = dict(arch='figsr', synth=kw, seed=seed, probe=results, one_block=one_block, gray=gray, uneven_halves=uneven, torch=torch.__version__,
                generator='tools/gen_golden_figsr.py')  # fmt: skip
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **arrays)
    print(name, json.dumps(meta, indent=1))


if __name__ == '__main__':
    main()
