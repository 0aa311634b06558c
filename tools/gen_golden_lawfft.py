#!/usr/bin/env python3
"""Generate the LAWFFT golden fixtures (tests/golden/lawfft_*.npz) by running the REAL reference on the CPU.

Imports tools/gen_golden.py for its import shims; LAWFFT's private DySample also calls ``torch.tensor(..., pin_memory=True)``
(lawfft/arch.py:66), so the same no-pin shim is installed on that module.  Writes only files with the prefix above.  Each fixture records
the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred, the hyper-parameters it handed to the module
(captured at the call), the uid of every reference architecture that claims the state dict (``claimed_by`` the first, ``claims`` all), the
names, shapes and dtypes of the reference module's state_dict -- no weights -- and ``f64_dev``, the deviation of the reference's own f32
forward from its forward on a ``.double()`` copy (whose FSAS still transforms in f32, as the module is written: ``q.float()``), with
``y_absmax`` to read it against.  The file round trip through the reference's own loader (``.pth``) is part of every case.

``lawfft_probe.npz`` holds only the probe of where the reference itself refuses: the input sizes around the reflect pad's limit, an
``unshuffle_mod`` checkpoint (through the registry, and handed to the loader and its module's ``load_state_dict`` directly), the (dim, local) pairs whose float ``split`` lands
on ``local - 1`` (found by enumeration; the first is loaded), and an ``n_mblock = 1`` checkpoint.

Usage:  python tools/gen_golden_lawfft.py
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

import resselt.archs.lawfft as _pkg  # noqa: E402

S = dict(dim=32, local=8, n_rblock=1, n_mblock=2)
CASES = [  # name, synth kwargs, input shape, seed
    ('lawfft_x4_psd_d60_r4_m6_9x11', dict(), (1, 3, 9, 11), 1501),  # the default model: 60 / 15 / 45, nothing a multiple of 8; one past 8 x 8
    ('lawfft_x2_psd_d32_r1_m2_n2_8x16', dict(S, scale=2), (2, 3, 8, 16), 1502),  # batch 2; already a multiple of 8
    ('lawfft_x3_ps_d64_m16_r1_m3_9x17', dict(dim=64, local=16, n_rblock=1, n_mblock=3, scale=3, upsampler='pixelshuffle', mid_dim=16), (1, 3, 9, 17), 1503),  # 64 / 16 / 48; an even last block
    ('lawfft_x4_nc_d32_r1_m2_7x10', dict(S, scale=4, upsampler='nearest+conv'), (1, 3, 7, 10), 1504),
    ('lawfft_x2_dys_d32_m16_r2_m2_6x9', dict(S, n_rblock=2, scale=2, upsampler='dysample', mid_dim=16), (1, 3, 6, 9), 1505),
    ('lawfft_x3_dys_d32_m32_r1_m2_10x7', dict(S, scale=3, upsampler='dysample', mid_dim=32), (1, 3, 10, 7), 1506),  # DySample on the features themselves
    ('lawfft_x1_conv_d32_r1_m2_11x13', dict(S, scale=1, upsampler='conv'), (1, 3, 11, 13), 1507),
    ('lawfft_x2_psd_d40_t0625_mlp2_r1_m2_9x9', dict(dim=40, local=8, n_rblock=1, n_mblock=2, scale=2, t_mid_factor=0.625, mlp_factor=2.0), (1, 3, 9, 9), 1508),  # FSAS width 20 of 32, hidden 80
    ('lawfft_x4_ps_d32_m16_r1_m2_7x6', dict(S, scale=4, upsampler='pixelshuffle', mid_dim=16), (1, 3, 7, 6), 1509),  # two shuffle stages
    ('lawfft_x2_nc_d60_r1_m3_n2_9x8', dict(dim=60, local=15, n_rblock=1, n_mblock=3, scale=2, upsampler='nearest+conv'), (2, 3, 9, 8), 1510),
    ('lawfft_x3_nc_d32_r1_m2_8x8', dict(S, scale=3, upsampler='nearest+conv'), (1, 3, 8, 8), 1511),
]  # fmt: skip
PROBE = ('lawfft_probe', dict(S, scale=2), ((4, 8), (8, 4), (3, 9), (5, 8), (8, 5), (8, 8), (9, 12)), 1520)

_captured: dict = {}
# the registered loader's own globals (the registry imports the architecture packages by walking the file system, so the module object
# it holds need not be the one ``import`` returns)
_arch = resselt.archs.internal_registry.get('LAWFFT')
_loader_globals = _arch.load.__func__.__globals__
_RealLAWFFT = _loader_globals['LAWFFT']
sys.modules[_RealLAWFFT.__module__].torch = G._TorchNoPin()


def _capture(**kw):
    _captured.clear()
    _captured.update(kw)
    return _RealLAWFFT(**kw)


_loader_globals['LAWFFT'] = _pkg.LAWFFT = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def load(sd):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'lawfft.pth')
        torch.save(dict(sd), path)
        return resselt.load_from_file(path).eval()


def _raises(fn) -> dict:
    try:
        fn()
        return dict(raises=None)
    except Exception as e:  # noqa: BLE001  (the probe records whatever the reference raises)
        return dict(raises=type(e).__name__, message=(str(e).splitlines() or [''])[0][:160])


def float_split_pairs(max_dim: int = 128) -> list:
    """(dim, local) with ``int((1 / (dim / local)) * dim) != local``: the reference's module then builds another local width than the
    checkpoint has."""
    return [(d, lo) for d in range(2, max_dim + 1) for lo in range(1, d) if int((1 / (d / lo)) * d) != lo]


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.lawfft_state_dict(seed=seed, **kw)
        model = load(sd)
        hyper = {k: (v if isinstance(v, (str, float, bool)) else int(v)) for k, v in _captured.items()}
        ref_sd = model.state_dict()
        assert list(ref_sd) == list(sd) and all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype and ref_sd[k].shape == v.shape for k, v in sd.items()), name
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double()(x.double())
        who = claims(sd)
        meta = dict(arch='lawfft', synth=kw, seed=seed, metadata=G.meta_of(model), hyper=hyper, claimed_by=who[0] if who else '', claims=who,
                    state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()),
                    torch=torch.__version__, generator='tools/gen_golden_lawfft.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        assert size <= 64 * 1024, (name, size)
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")

    name, kw, sizes, seed = PROBE
    model = load(synth.lawfft_state_dict(seed=seed, **kw))
    results, arrays = [], {}
    for h, w in sizes:
        x = synth.synth_input((1, 3, h, w), seed)
        r = _raises(lambda: arrays.__setitem__(f'y_{h}x{w}', model(x.clone()).detach().numpy()))
        if r['raises'] is None:
            arrays[f'x_{h}x{w}'] = x.numpy()
        results.append(dict(size=[h, w], **r))
    un_kw = dict(S, scale=2, unshuffle_mod=True)
    un_sd = synth.lawfft_state_dict(seed=seed, **un_kw)
    unshuffle = dict(synth=un_kw, claims=claims(un_sd), registry=_raises(lambda: resselt.load_from_state_dict(dict(un_sd))), loader=_raises(lambda: _arch.load(dict(un_sd)).load_state_dict(dict(un_sd))))
    pairs = float_split_pairs()
    d, lo = pairs[0]
    fs_kw = dict(dim=d, local=lo, n_rblock=1, n_mblock=2, scale=2)
    float_split = dict(pairs=[list(p) for p in pairs[:16]], count=len(pairs), synth=fs_kw, int_split_dim=int((1 / (d / lo)) * d),
                       **_raises(lambda: resselt.load_from_state_dict(dict(synth.lawfft_state_dict(seed=seed, **fs_kw)))))  # fmt: skip
    one_kw = dict(S, n_mblock=1, scale=2)
    one_block = dict(synth=one_kw, **_raises(lambda: resselt.load_from_state_dict(dict(synth.lawfft_state_dict(seed=seed, **one_kw)))))
    meta = dict(arch='lawfft', synth=kw, seed=seed, probe=results, unshuffle=unshuffle, float_split=float_split, one_block=one_block, torch=torch.__version__,
                generator='tools/gen_golden_lawfft.py')  # fmt: skip
    np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), **arrays)
    print(name, json.dumps(meta, indent=1))


if __name__ == '__main__':
    main()
