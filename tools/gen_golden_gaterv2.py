#!/usr/bin/env python3
"""Generate the GateRv2 golden fixtures (tests/golden/gaterv2_*.npz) by running the REAL reference on the CPU (nothing in GateRv2 differs
between training and eval mode; the module is put into eval mode all the same).

Imports tools/gen_golden.py for its import shims; GateRv2's private DySample also calls ``torch.tensor(..., pin_memory=True)``, so the same
no-pin shim is installed on that module.  Writes only files with the prefix above.

x1 cases go through the reference's loader.  Each records the synthetic checkpoint's arguments, the seed, the metadata the loader inferred,
the hyper-parameters it handed to the module (captured at the call), the uid of every reference architecture that claims the state dict
(``claimed_by`` the first, ``claims`` all), the names and shapes of the reference module's state_dict -- no weights -- and ``f64_dev``, the
deviation of the reference's own f32 forward from its forward on a ``.double()`` copy, with ``y_absmax`` to read it against.

Above x1 the reference's loader raises ``KeyError`` (it reads ``to_img.MetaUpsample``; the probe records it), and the reference module sets
``self.scale = 1`` whatever it is given, so it crops the upscaled image to the input's size.  Those cases are therefore generated from the
real reference module built directly with the generator's arguments, the checkpoint loaded with its own ``load_state_dict``, and its INSTANCE
attribute ``scale`` set to the true scale after construction; the fixture's metadata says so (``via``, ``scale_attribute_set``), ``hyper`` is
the generator's arguments and ``metadata`` what the loader's ``_enhance_model`` call would record with the true scale.

``gaterv2_probe.npz`` holds the probe: the loader's ``KeyError``, the unmodified module's (cropped) output for the x2 pixelshuffledirect
case, which input sides make the reference raise around the minimum for P = 4 and P = 16 (and what), input and output of those that run,
a checkpoint with more encoder than decoder levels, what a 'conv' head above x1 returns, and who claims a GateRv2 state dict.

Usage:  python tools/gen_golden_gaterv2.py
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

import resselt.archs.gaterv2 as _pkg  # noqa: E402

from resselt_amd.archs.gaterv2 import DETECTION_KEYS  # noqa: E402

SMALL = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=2)
CASES = [  # name, synth kwargs, input shape, seed
    ('gaterv2_x1_default_17x35', dict(), (1, 3, 17, 35), 1601),  # (2, 2, 4, 6) / (2, 2, 2, 2), 10 latent blocks at 768 channels, m = 48; 2 x 3 tokens
    ('gaterv2_x1_d8_l2_5x6', dict(**SMALL), (1, 3, 5, 6), 1602),  # latent width 32, m = 2: not a multiple of 8
    ('gaterv2_x1_d24_l2_9x7', dict(dim=24, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=2), (1, 3, 9, 7), 1603),  # m = 6
    ('gaterv2_x1_d16_l4_16x32', dict(dim=16, enc_blocks=(1, 1, 1, 1), dec_blocks=(1, 1, 1, 1), num_latent=2), (1, 3, 16, 32), 1604),  # m = 16; sides exactly P and 2 P
    ('gaterv2_x1_d8_l2_chunks_45x50', dict(**SMALL), (1, 3, 45, 50), 1605),  # 12 x 13 = 156 tokens: two chunks, the last one ragged
    ('gaterv2_x1_d8_b2_6x5', dict(**SMALL), (2, 3, 6, 5), 1606),  # batch 2: sca's mean and the attention are per image
    ('gaterv2_x1_gray_d8_7x9', dict(in_ch=1, **SMALL), (1, 1, 7, 9), 1607),
    ('gaterv2_x1_unequal_d8_l3_9x11', dict(dim=8, enc_blocks=(1, 3, 2), dec_blocks=(2, 1, 3), num_latent=3), (1, 3, 9, 11), 1608),  # P = 8; side 9: pad 7, the largest legal
    ('gaterv2_x2_psd_d8_5x7', dict(scale=2, upsample='pixelshuffledirect', **SMALL), (1, 3, 5, 7), 1609),
    ('gaterv2_x3_psd_d8_6x5', dict(scale=3, upsample='pixelshuffledirect', **SMALL), (1, 3, 6, 5), 1610),
    ('gaterv2_x4_ps_d16_7x4', dict(scale=4, upsample='pixelshuffle', upsample_mid_dim=16, dim=16, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1), (1, 3, 7, 4), 1611),  # a side exactly P
    ('gaterv2_x3_ps_d8_4x5', dict(scale=3, upsample='pixelshuffle', upsample_mid_dim=8, **SMALL), (1, 3, 4, 5), 1612),  # side 5: the largest legal pad for P = 4
    ('gaterv2_x4_nc_d8_5x3', dict(scale=4, upsample='nearest+conv', **SMALL), (1, 3, 5, 3), 1613),  # side 3: the smallest that runs
    ('gaterv2_x3_nc_d8_4x6', dict(scale=3, upsample='nearest+conv', **SMALL), (1, 3, 4, 6), 1614),
    ('gaterv2_x2_dys_d8_6x7', dict(scale=2, upsample='dysample', upsample_mid_dim=16, **SMALL), (1, 3, 6, 7), 1615),  # (UniUpsample v1: no front convolution whatever mid_dim)
    ('gaterv2_x3_dys_d8_4x4', dict(scale=3, upsample='dysample', **SMALL), (1, 3, 4, 4), 1616),
    ('gaterv2_x2_conv_d8_5x6', dict(scale=2, upsample='conv', **SMALL), (1, 3, 5, 6), 1617),  # does not upsample: the padded 8 x 8 map, cropped to at most 10 x 12
]  # fmt: skip
CROP_CASE = 'gaterv2_x2_psd_d8_5x7'
PROBE2 = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1)  # P = 4
PROBE4 = dict(dim=8, enc_blocks=(1, 1, 1, 1), dec_blocks=(1, 1, 1, 1), num_latent=1)  # P = 16
PROBE_SEED = 1620
ARGS = ('in_ch', 'dim', 'enc_blocks', 'dec_blocks', 'num_latent', 'scale', 'upsample', 'upsample_mid_dim')

_captured: dict = {}
_arch = resselt.archs.internal_registry.get('GateRv2')
_loader_globals = _arch.load.__func__.__globals__
_Real = _loader_globals['GateRV2']
sys.modules[_Real.__module__].torch = G._TorchNoPin()


def _capture(*args, **kw):
    _captured.clear()
    _captured.update(dict(zip(ARGS, args)), **kw)
    return _Real(*args, **kw)


_loader_globals['GateRV2'] = _pkg.GateRV2 = _capture  # the loader's call site: what it inferred, as it hands it over


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def load(sd):
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        path = os.path.join(tmp, 'gaterv2.pth')
        torch.save(dict(sd), path)
        return resselt.load_from_file(path)


def build(kw, sd, set_scale=True):
    """The real reference module from the generator's arguments with the checkpoint loaded; ``set_scale``: its instance attribute ``scale``
    set to the true scale (the constructor leaves it at 1)."""
    defaults = dict(in_ch=3, dim=48, enc_blocks=(2, 2, 4, 6), dec_blocks=(2, 2, 2, 2), num_latent=10, scale=1, upsample='pixelshuffledirect', upsample_mid_dim=32)
    hyper = {k: kw.get(k, defaults[k]) for k in ARGS}
    model = _Real(**hyper)
    model.load_state_dict(dict(sd))
    assert model.scale == 1  # the defect: whatever ``scale`` was given
    if set_scale:
        model.scale = hyper['scale']
    return model.eval(), hyper


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
        sd = synth.gaterv2_state_dict(seed=seed, **kw)
        above = kw.get('scale', 1) != 1
        if above:
            model, hyper = build(kw, sd)
            hyper = _plain(hyper)
            md = dict(in_channels=hyper['in_ch'], out_channels=hyper['in_ch'], upscale=hyper['scale'], name='GateRv2', cls=type(model).__name__)
            via = 'module built directly; the reference loader raises KeyError above x1'
        else:
            model = load(sd)
            hyper, md = _plain(_captured), G.meta_of(model)
            model = model.eval()
            via = 'the reference loader'
        ref_sd = model.state_dict()
        assert list(ref_sd) == list(sd), name
        assert all(torch.equal(ref_sd[k], v) and ref_sd[k].dtype == v.dtype for k, v in sd.items() if not k.endswith('MetaUpsample')), name
        x = synth.synth_input(shape, seed)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            y = model(x.clone())
            m64 = copy.deepcopy(model).double().eval()
            m64.scale = model.scale
            y64 = m64(x.double())
        who = claims(sd)
        assert who, name
        meta = dict(arch='gaterv2', synth=_plain(kw), seed=seed, metadata=md, hyper=hyper, claimed_by=who[0], claims=who, via=via,
                    scale_attribute_set=bool(above), state_dict={k: list(v.shape) for k, v in ref_sd.items()},
                    dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()), mode='eval',
                    torch=torch.__version__, generator='tools/gen_golden_gaterv2.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        assert size <= 64 * 1024, (name, size)
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  hyper {hyper}  {size} B")

    results, arrays = [], {}
    for tag, kw, sides in (('p4', PROBE2, (1, 2, 3, 4, 5)), ('p16', PROBE4, (8, 9, 16, 17))):
        model = load(synth.gaterv2_state_dict(seed=PROBE_SEED, **kw)).eval()
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
    # the loader above x1, and the module's own crop
    name, kw, shape, seed = next(c for c in CASES if c[0] == CROP_CASE)
    sd = synth.gaterv2_state_dict(seed=seed, **kw)
    loader = dict(error_of(lambda: load(sd)), claims=claims(sd), case=name)
    plain, _ = build(kw, sd, set_scale=False)
    x = synth.synth_input(shape, seed)
    with torch.no_grad():
        y_plain = plain(x.clone())
    arrays['x_crop'], arrays['y_crop_unmodified'] = x.numpy(), y_plain.numpy()
    crop = dict(case=name, scale_attribute=int(plain.scale), scale_argument=int(kw['scale']), x=list(x.shape), y_unmodified=list(y_plain.shape))
    # more encoder than decoder levels (a checkpoint needs two of each to be detected)
    dec_kw = dict(dim=8, enc_blocks=(1, 1, 1), dec_blocks=(1, 1), num_latent=1)
    dec_sd = synth.gaterv2_state_dict(seed=PROBE_SEED, **dec_kw)
    dec_load = error_of(lambda: load(dec_sd))
    dec_fwd = error_of(lambda: load(dec_sd).eval()(synth.synth_input((1, 3, 16, 16), PROBE_SEED))) if dec_load['raises'] is None else None
    one_kw = dict(dim=8, enc_blocks=(1,), dec_blocks=(1,), num_latent=1)
    one_sd = synth.gaterv2_state_dict(seed=PROBE_SEED, **one_kw)
    one = dict(synth=_plain(one_kw), claims=claims(one_sd), **error_of(lambda: resselt.load_from_state_dict(dict(one_sd))))
    # a 'conv' head above x1: the module as it is, and with the true scale
    cname, ckw, cshape, cseed = next(c for c in CASES if c[0] == 'gaterv2_x2_conv_d8_5x6')
    csd = synth.gaterv2_state_dict(seed=cseed, **ckw)
    cx = synth.synth_input(cshape, cseed)
    with torch.no_grad():
        c_plain, c_set = build(ckw, csd, set_scale=False)[0](cx.clone()), build(ckw, csd)[0](cx.clone())
    conv = dict(case=cname, x=list(cx.shape), y_unmodified=list(c_plain.shape), y_scale_set=list(c_set.shape),
                corner_equal=bool(torch.equal(c_set[:, :, : cshape[2], : cshape[3]], c_plain)))  # fmt: skip
    p4_sd = synth.gaterv2_state_dict(seed=PROBE_SEED, **PROBE2)
    ref_keys = [k for k in DETECTION_KEYS if not _arch.detect({q: v for q, v in p4_sd.items() if q != k})]
    meta = dict(arch='gaterv2', seed=PROBE_SEED, synth=dict(p4=_plain(PROBE2), p16=_plain(PROBE4)), probe=results, loader_above_x1=loader, scale_crop=crop,
                dec_ne_enc=dict(synth=_plain(dec_kw), load=dec_load, forward=dec_fwd), one_level=one, conv_above_x1=conv, x1_claims=claims(p4_sd),
                detection_keys_needed=len(ref_keys), detection_keys=len(DETECTION_KEYS), p4_keys=len(p4_sd), torch=torch.__version__,
                generator='tools/gen_golden_gaterv2.py')  # fmt: skip
    np.savez_compressed(os.path.join(G.OUT, 'gaterv2_probe.npz'), meta=np.array(json.dumps(meta)), **arrays)
    print('gaterv2_probe', json.dumps(meta, indent=1)[:4000], os.path.getsize(os.path.join(G.OUT, 'gaterv2_probe.npz')))


if __name__ == '__main__':
    main()
