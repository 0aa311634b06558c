#!/usr/bin/env python3
"""Generate the GateRV3 golden fixtures (tests/golden/gaterv3_*.npz) by running the REAL reference on the CPU, in eval mode (the
reference's loader returns training mode, where ``sisr_end_conv`` differs from its fold on the border ring; the engine computes eval mode).

Imports tools/gen_golden.py for its import shims; GateRV3's private DySample also calls ``torch.tensor(..., pin_memory=True)``, so the same
no-pin shim is installed on that module.  ``LDA_AQU`` and the reference's ``load_state_dict`` print: silenced.  Writes only files with the
prefix above.  Each fixture records the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred, the
hyper-parameters it handed to the module (captured at the call), the uid of every reference architecture that claims the state dict
(``claimed_by`` the first, ``claims`` all), the names and shapes of the reference module's state_dict -- no weights -- and ``f64_dev``, the
deviation of the reference's own f32 forward from its forward on a ``.double()`` copy, with ``y_absmax`` to read it against.  The stored
``eval_conv.*`` tensors are placeholders that ``eval()`` overwrites with the fold, so they are left out of the round-trip comparison.

``gaterv3_probe.npz`` holds the probe: which input sides make the reference raise around the minimum for P = 4 and P = 16 (and what),
input and output of those that run, the failure of a checkpoint with more encoder than decoder levels, the non-detection of one with
``span_blocks = 0``, the attention's assertion, and what a 'conv' head above x1 does.

Usage:  python tools/gen_golden_gaterv3.py
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

import resselt.archs.gaterv3 as _pkg  # noqa: E402

SMALL = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=2, span_blocks=1)
CASES = [  # name, synth kwargs, input shape, seed
    ('gaterv3_x1_default_17x35', dict(), (1, 3, 17, 35), 1501),  # (2, 2, 4, 8) / (2, 2, 2, 2), 12 latent blocks, four span blocks; pad 15 and 13
    ('gaterv3_x1_att_hd1_d8_l1_5x6', dict(dim=8, enc_blocks=(2,), dec_blocks=(1,), num_latent=2, span_blocks=1, attention=True), (1, 3, 5, 6), 1502),
    ('gaterv3_x1_att_hd4_d16_l2_9x7', dict(dim=16, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=2, span_blocks=1, attention=True), (1, 3, 9, 7), 1503),
    ('gaterv3_x1_att_hd32_d32_l4_16x32', dict(enc_blocks=(1, 1, 1, 1), dec_blocks=(1, 1, 1, 1), num_latent=2, span_blocks=1, attention=True), (1, 3, 16, 32), 1504),  # sides exactly P and 2 P
    ('gaterv3_x2_psd_d8_5x7', dict(scale=2, upsample='pixelshuffledirect', **SMALL), (1, 3, 5, 7), 1505),
    ('gaterv3_x3_psd_d8_6x5', dict(scale=3, upsample='pixelshuffledirect', **SMALL), (1, 3, 6, 5), 1506),
    ('gaterv3_x4_ps_d16_7x4', dict(scale=4, upsample='pixelshuffle', upsample_mid_dim=16, dim=16, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1, span_blocks=1), (1, 3, 7, 4), 1507),  # a side exactly P
    ('gaterv3_x3_ps_d8_4x5', dict(scale=3, upsample='pixelshuffle', upsample_mid_dim=8, **SMALL), (1, 3, 4, 5), 1508),  # side 5: the largest legal pad for P = 4
    ('gaterv3_x4_nc_d8_5x3', dict(scale=4, upsample='nearest+conv', **SMALL), (1, 3, 5, 3), 1509),  # side 3: the smallest that runs
    ('gaterv3_x3_nc_d8_4x6', dict(scale=3, upsample='nearest+conv', **SMALL), (1, 3, 4, 6), 1510),
    ('gaterv3_x2_dys_front_k3_d8_6x7', dict(scale=2, upsample='dysample', upsample_mid_dim=16, end_kernel=3, **SMALL), (1, 3, 6, 7), 1511),
    ('gaterv3_x2_dys_front_k1_d8_5x4', dict(scale=2, upsample='dysample', upsample_mid_dim=16, end_kernel=1, **SMALL), (1, 3, 5, 4), 1512),
    ('gaterv3_x3_dys_k1_d8_4x4', dict(scale=3, upsample='dysample', upsample_mid_dim=8, end_kernel=1, **SMALL), (1, 3, 4, 4), 1513),  # mid_dim = dim: no front convolution
    ('gaterv3_x4_dys_k3_d16_3x5', dict(scale=4, upsample='dysample', upsample_mid_dim=16, end_kernel=3, dim=16, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1, span_blocks=2), (1, 3, 3, 5), 1514),
    ('gaterv3_x1_gray_d8_7x9', dict(in_ch=1, **SMALL), (1, 1, 7, 9), 1515),
    ('gaterv3_x2_psd_d8_b2_6x5', dict(scale=2, upsample='pixelshuffledirect', **SMALL), (2, 3, 6, 5), 1516),  # batch 2: sca's mean is per image
    ('gaterv3_x1_unequal_d8_l3_9x11', dict(dim=8, enc_blocks=(1, 3, 2), dec_blocks=(2, 1, 3), num_latent=3, span_blocks=3), (1, 3, 9, 11), 1517),  # P = 8; side 9: pad 7, the largest legal
    ('gaterv3_x1_nogamma_d8_8x8', dict(with_gamma=False, **SMALL), (1, 3, 8, 8), 1518),  # a missing gamma means ones
]  # fmt: skip
PROBE2 = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1, span_blocks=1)  # P = 4
PROBE4 = dict(dim=8, enc_blocks=(1, 1, 1, 1), dec_blocks=(1, 1, 1, 1), num_latent=1, span_blocks=1)  # P = 16
PROBE_SEED = 1520

_captured: dict = {}
_loader_globals = resselt.archs.internal_registry.get('GateRV3').load.__func__.__globals__
_Real = _loader_globals['GateRV3']
sys.modules[_Real.__module__].torch = G._TorchNoPin()


def _capture(*args, **kw):
    names = ('in_ch', 'dim', 'enc_blocks', 'dec_blocks', 'num_latent', 'scale', 'upsample', 'upsample_mid_dim')
    _captured.clear()
    _captured.update(dict(zip(names, args)), **kw)
    return _Real(*args, **kw)


_loader_globals['GateRV3'] = _pkg.GateRV3 = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def load(sd):
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        path = os.path.join(tmp, 'gaterv3.pth')
        torch.save(dict(sd), path)
        return resselt.load_from_file(path)


def _plain(d):
    out = {}
    for k, v in d.items():
        out[k] = [int(t) for t in v] if isinstance(v, (list, tuple)) else (v if isinstance(v, (str, float, bool)) else int(v))
    return out


def error_of(fn) -> dict:
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
    except Exception as e:  # noqa: BLE001  (the probe records whatever the reference raises)
        return dict(raises=type(e).__name__, message=str(e).strip().splitlines()[0][:160] if str(e).strip() else '')
    return dict(raises=None)


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.gaterv3_state_dict(seed=seed, **kw)
        model = load(sd)
        hyper, md = _plain(_captured), G.meta_of(model)
        ref_sd = model.state_dict()
        want = list(sd) if 'gamma' in sd else ['gamma'] + list(sd)
        assert list(ref_sd) == want, name
        assert all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype for k, v in sd.items() if 'eval_conv' not in k and not k.endswith('MetaUpsample')), name
        model = model.eval()
        x = synth.synth_input(shape, seed)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            y = model(x.clone())
            y64 = copy.deepcopy(model).double().eval()(x.double())
        who = claims(sd)
        assert who, name
        meta = dict(arch='gaterv3', synth=_plain(kw), seed=seed, metadata=md, hyper=hyper, claimed_by=who[0], claims=who,
                    state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()), mode='eval',
                    torch=torch.__version__, generator='tools/gen_golden_gaterv3.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        assert size <= 64 * 1024, (name, size)
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")

    results, arrays = [], {}
    for tag, kw, sides in (('p4', PROBE2, (1, 2, 3, 4, 5)), ('p16', PROBE4, (8, 9, 16, 17))):
        model = load(synth.gaterv3_state_dict(seed=PROBE_SEED, **kw)).eval()
        for side in sides:
            for h, w in ((side, 2 * side + 3), (2 * side + 3, side)) if side < 16 else ((side, side),):
                x = synth.synth_input((1, 3, h, w), PROBE_SEED)
                out = {}

                def run(x=x, out=out, model=model):
                    with torch.no_grad():
                        out['y'] = model(x.clone())

                res = error_of(run)
                results.append(dict(model=tag, size=[h, w], **res))
                if res['raises'] is None and h * w <= 400:
                    arrays[f'x_{tag}_{h}x{w}'], arrays[f'y_{tag}_{h}x{w}'] = x.numpy(), out['y'].numpy()
    dec_kw = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1,), num_latent=1, span_blocks=1)
    dec_sd = synth.gaterv3_state_dict(seed=PROBE_SEED, **dec_kw)
    dec_load = error_of(lambda: load(dec_sd))
    dec_fwd = error_of(lambda: load(dec_sd).eval()(synth.synth_input((1, 3, 8, 8), PROBE_SEED))) if dec_load['raises'] is None else None
    span_kw = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1, span_blocks=0)
    span_sd = synth.gaterv3_state_dict(seed=PROBE_SEED, **span_kw)
    span0 = error_of(lambda: resselt.load_from_state_dict(dict(span_sd)))
    conv_kw = dict(scale=2, upsample='conv', **SMALL)  # UniUpsampleV3's 'conv' does not upsample: the shortcut's size cannot match above x1
    conv_sd = synth.gaterv3_state_dict(seed=PROBE_SEED, **conv_kw)
    conv2 = error_of(lambda: load(conv_sd).eval()(synth.synth_input((1, 3, 8, 8), PROBE_SEED)))
    att = error_of(lambda: _Real(3, 12, (1,), (1,), 1, attention=True))
    detect = sorted(k for k in synth.gaterv3_state_dict(seed=PROBE_SEED, **PROBE2) if k != 'gamma')
    meta = dict(arch='gaterv3', seed=PROBE_SEED, synth=dict(p4=_plain(PROBE2), p16=_plain(PROBE4)), probe=results,
                dec_ne_enc=dict(synth=_plain(dec_kw), load=dec_load, forward=dec_fwd), span_blocks_0=dict(synth=_plain(span_kw), claims=claims(span_sd), **span0),
                attention_assert=dict(args='in_ch=3, dim=12, enc_blocks=(1,), dec_blocks=(1,), num_latent=1, attention=True', **att),
                conv_above_x1=dict(synth=_plain(conv_kw), **conv2), p4_keys=len(detect), torch=torch.__version__, generator='tools/gen_golden_gaterv3.py')  # fmt: skip
    np.savez_compressed(os.path.join(G.OUT, 'gaterv3_probe.npz'), meta=np.array(json.dumps(meta)), **arrays)
    print('gaterv3_probe', json.dumps(meta, indent=1)[:3000], os.path.getsize(os.path.join(G.OUT, 'gaterv3_probe.npz')))


if __name__ == '__main__':
    main()
