#!/usr/bin/env python3
"""Generate the GFISR (v1) golden fixtures (tests/golden/gfisr_*.npz) by running the REAL reference on the CPU, in eval mode: the
FourierUnit's reflect pad exists only there (``train(False)`` sets it).

Imports tools/gen_golden.py for its import shims; GFISR's private DySample also calls ``torch.tensor(..., pin_memory=True)``, so the same
no-pin shim is installed on that module.  The reference's ``load_state_dict`` prints the MetaUpsample buffer: silenced.  Writes only files
with the prefix above.  Each fixture records the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred,
the hyper-parameters it handed to the module (captured at the call), the uid of every reference architecture that claims the state dict
(``claimed_by`` the first, ``claims`` all), the names, shapes and dtypes of the reference module's state_dict -- no weights -- and
``f64_dev``, the deviation of the reference's own f32 forward from its forward on a ``.double()`` copy (whose FourierUnit still transforms
in f32, as the module is written), with ``y_absmax`` to read it against.  The file round trip through the reference's own loader
(``.pth``) is part of every loader case.  The ``DIRECT`` cases are ``pixel_unshuffle`` models, which the reference's loader cannot
produce (its detection needs ``in_to_dim.weight``): the module is built directly and ``claims`` is recorded as it comes out, empty.

``gfisr_probe.npz`` holds the probe: which of the feature grids 3x3, 3x4, 4x3, 4x4, 4x5 and 5x5 make the reference raise (and what), input
and output of those that run, the error of a checkpoint whose head has ``mid_dim != 32``, and what happens to a ``pixel_unshuffle``
checkpoint.

Usage:  python tools/gen_golden_gfisr.py
"""

from __future__ import annotations

import contextlib
import copy
import io
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth

import resselt.archs.gfisr as _pkg  # noqa: E402

CASES = [  # name, synth kwargs, input shape, seed
    ('gfisr_x4_psd_d48_b24_9x11', dict(), (1, 3, 9, 11), 1401),  # the default model; odd x odd
    ('gfisr_x2_psd_d16_b6_b2_6x8', dict(dim=16, n_blocks=6, scale=2), (2, 3, 6, 8), 1402),  # all five rotations and one wrap; batch 2
    ('gfisr_x3_ps_d24_b5_7x10', dict(dim=24, n_blocks=5, scale=3, upsampler='pixelshuffle'), (1, 3, 7, 10), 1403),  # odd x even
    ('gfisr_x4_nc_d64_b2_8x5', dict(dim=64, n_blocks=2, scale=4, upsampler='nearest+conv'), (1, 3, 8, 5), 1404),
    ('gfisr_x2_dys_d16_b2_5x7', dict(dim=16, n_blocks=2, scale=2, upsampler='dysample'), (1, 3, 5, 7), 1405),  # mid_dim 32 != dim: front convolution
    ('gfisr_x3_dys_d32_b1_6x5', dict(dim=32, n_blocks=1, scale=3, upsampler='dysample'), (1, 3, 6, 5), 1406),  # mid_dim = dim: none
    ('gfisr_x1_conv_d16_gray_b4_11x13', dict(dim=16, n_blocks=4, scale=1, upsampler='conv', in_nc=1, out_nc=1), (1, 1, 11, 13), 1407),
    ('gfisr_x2_psd_d48_e15_b2_4x6', dict(dim=48, n_blocks=2, scale=2, expansion_ratio=1.5), (1, 3, 4, 6), 1408),
    ('gfisr_x4_psd_d8_b5_4x4', dict(dim=8, n_blocks=5, scale=4), (1, 3, 4, 4), 1409),  # gc = 1: two spectral channels
    ('gfisr_x3_psd_d16_nofft_b5_4x3', dict(dim=16, n_blocks=5, scale=3, fft_mode=False), (1, 3, 4, 3), 1410),  # no pad, no minimum size
]  # fmt: skip
DIRECT = [  # pixel_unshuffle models: the feature grid is 4 x 5 in both
    ('gfisr_x2_pu_d16_b5_7x9', dict(dim=16, n_blocks=5, scale=2, pixel_unshuffle=True), (1, 3, 7, 9), 1411),
    ('gfisr_x1_pu_d16_b5_14x18', dict(dim=16, n_blocks=5, scale=1, pixel_unshuffle=True), (1, 3, 14, 18), 1412),
]
PROBE = ('gfisr_probe', dict(dim=16, n_blocks=1, scale=2), ((3, 3), (3, 4), (4, 3), (4, 4), (4, 5), (5, 5)), 1420)

_captured: dict = {}
# the registered loader's own globals (the registry imports the architecture packages by walking the file system, so the module object
# it holds need not be the one ``import`` returns)
_loader_globals = resselt.archs.internal_registry.get('GFISR').load.__func__.__globals__
_RealGFISR = _loader_globals['GFISR']
sys.modules[_RealGFISR.__module__].torch = G._TorchNoPin()


def _capture(**kw):
    _captured.clear()
    _captured.update(kw)
    return _RealGFISR(**kw)


_loader_globals['GFISR'] = _pkg.GFISR = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def load(sd):
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        path = os.path.join(tmp, 'gfisr.pth')
        torch.save(dict(sd), path)
        return resselt.load_from_file(path).eval()


def build(sd, kw):
    """A model the loader cannot produce: the reference module itself, from the synthetic checkpoint's own arguments."""
    with contextlib.redirect_stdout(io.StringIO()):
        model = _RealGFISR(**{k: v for k, v in kw.items()})
        model.load_state_dict(dict(sd))
    return model.eval()


def _plain(d):
    return {k: (v if isinstance(v, (str, float, bool)) else int(v)) for k, v in d.items()}


def error_of(fn) -> dict:
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
    except Exception as e:  # noqa: BLE001  (the probe records whatever the reference raises)
        return dict(raises=type(e).__name__, message=str(e).strip().splitlines()[0][:160] if str(e).strip() else '')
    return dict(raises=None)


def main():
    for direct, cases in ((False, CASES), (True, DIRECT)):
        for name, kw, shape, seed in cases:
            sd = synth.gfisr_state_dict(seed=seed, **kw)
            if direct:
                model, hyper, md = build(sd, kw), _plain(kw), None
            else:
                model = load(sd)
                hyper, md = _plain(_captured), G.meta_of(model)
            ref_sd = model.state_dict()
            assert list(ref_sd) == list(sd) and all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype for k, v in sd.items()), name
            x = synth.synth_input(shape, seed)
            with torch.no_grad():
                y = model(x.clone())
                y64 = copy.deepcopy(model).double().eval()(x.double())
            who = claims(sd)
            assert bool(who) != direct, (name, who)
            meta = dict(arch='gfisr', synth=kw, seed=seed, metadata=md, hyper=hyper, direct=direct, claimed_by=who[0] if who else '', claims=who,
                        state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                        y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()),
                        torch=torch.__version__, generator='tools/gen_golden_gfisr.py')  # fmt: skip
            np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
            size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
            assert size <= 64 * 1024, (name, size)
            print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")

    name, kw, sizes, seed = PROBE
    model = load(synth.gfisr_state_dict(seed=seed, **kw))
    results, arrays = [], {}
    for h, w in sizes:
        x = synth.synth_input((1, 3, h, w), seed)
        out = {}

        def run(x=x, out=out):
            with torch.no_grad():
                out['y'] = model(x.clone())

        res = error_of(run)
        results.append(dict(size=[h, w], **res))
        if res['raises'] is None:
            arrays[f'x_{h}x{w}'], arrays[f'y_{h}x{w}'] = x.numpy(), out['y'].numpy()
    mid_kw = dict(dim=16, n_blocks=1, scale=2, upsampler='pixelshuffle', mid_dim=16)
    mid = error_of(lambda: resselt.load_from_state_dict(dict(synth.gfisr_state_dict(seed=seed, **mid_kw))))
    pu_kw = dict(dim=16, n_blocks=1, scale=2, pixel_unshuffle=True)
    pu_sd = synth.gfisr_state_dict(seed=seed, **pu_kw)
    pu = error_of(lambda: resselt.load_from_state_dict(dict(pu_sd)))
    meta = dict(arch='gfisr', synth=kw, seed=seed, probe=results, mid_dim=dict(synth=mid_kw, **mid), pixel_unshuffle=dict(synth=pu_kw, claims=claims(pu_sd), **pu),
                torch=torch.__version__, generator='tools/gen_golden_gfisr.py')  # fmt: skip
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **arrays)
    print(name, results, meta['mid_dim'], meta['pixel_unshuffle'])


if __name__ == '__main__':
    main()
