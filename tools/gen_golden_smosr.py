#!/usr/bin/env python3
"""Generate the SMoSR golden fixtures (tests/golden/smosr_*.npz) by running the REAL reference on the CPU.

Imports tools/gen_golden.py for its import shims (the ``dysample`` head's ``pin_memory=True`` among them).  Writes only files with the
prefix above.  Each fixture records the synthetic checkpoint's arguments, the seed, the metadata the reference's loader inferred, the
hyper-parameters it handed to the module (captured at the call), the uid of every reference architecture that claims the state dict
(``claimed_by`` the first, ``claims`` all), the names, shapes and dtypes of the reference module's state_dict -- no weights --, the ``MetaUpsample`` buffer of a
freshly constructed reference module (``meta_upsample``), ``f64_dev``,
the reference's own f32-against-f64 deviation on the case, with ``y_absmax`` to read it against, and two statistics of the gate
pre-activations (the second half of every SMB's ``body`` output): their median magnitude and the share above 3, where tanh is flat.
The file round trip through the reference's own loader (``.pth``) is part of every case.

Usage:  python tools/gen_golden_smosr.py
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

import resselt.archs.smosr as _pkg  # noqa: E402

PA4 = dict(scale=4, rep=True, upsampler='pa_up', upsampler_mid_dim=32)
# head_gain: what brings |y|max of the case to order 1 (the last layer is linear).  The seeds are ones on which the gates stay in tanh's
# working range: tests/test_smosr_oracle.py asserts the recorded statistics of every fixture.
CASES = [  # name, synth kwargs, input shape, seed
    ('smosr_x2_psd_d48_rep0_9x11', dict(head_gain=4.0), (1, 3, 9, 11), 1213),
    ('smosr_x2_psd_d48_rep1_9x11', dict(rep=True, head_gain=8.0), (1, 3, 9, 11), 1202),
    ('smosr_x4_pa_d48_rep1_m32_8x9', dict(PA4, head_gain=128.0), (1, 3, 8, 9), 1203),
    ('smosr_x3_pa_d32_rep0_m24_n1_7x8', dict(scale=3, dim=32, n_mb=1, upsampler='pa_up', upsampler_mid_dim=24, head_gain=24.0), (2, 3, 7, 8), 1204),
    ('smosr_x3_ps_d48_m16_5x6', dict(scale=3, upsampler='pixelshuffle', upsampler_mid_dim=16, head_gain=8.0), (1, 3, 5, 6), 1205),
    ('smosr_x4_nc_d48_5x6', dict(scale=4, upsampler='nearest+conv', head_gain=24.0), (1, 3, 5, 6), 1206),
    ('smosr_x2_nc_d48_rep1_6x7', dict(scale=2, rep=True, upsampler='nearest+conv', head_gain=32.0), (1, 3, 6, 7), 1207),
    ('smosr_x2_dys_d48_m32_k3_6x7', dict(upsampler='dysample', upsampler_mid_dim=32, d_kernel=3, head_gain=12.0), (1, 3, 6, 7), 1208),
    ('smosr_x2_dys_d48_m32_k1_6x7', dict(upsampler='dysample', upsampler_mid_dim=32, d_kernel=1, head_gain=16.0), (1, 3, 6, 7), 1209),
    ('smosr_x1_conv_d48_3x4', dict(scale=1, upsampler='conv', head_gain=8.0), (1, 3, 3, 4), 1210),
    ('smosr_x2_psd_d24_gray_4x5', dict(in_ch=1, out_ch=1, dim=24, head_gain=4.0), (1, 1, 4, 5), 1211),
    # hidden head widths that are no multiple of 8 (pixelshuffle) or whose DySample groups are no multiple of 4 channels
    ('smosr_x4_ps_d16_m20_n1_5x6', dict(dim=16, n_mb=1, scale=4, upsampler='pixelshuffle', upsampler_mid_dim=20, head_gain=8.0), (2, 3, 5, 6), 1221),
    ('smosr_x2_dys_d16_m12_k1_n1_6x7', dict(dim=16, n_mb=1, upsampler='dysample', upsampler_mid_dim=12, d_kernel=1, head_gain=16.0), (2, 3, 6, 7), 1222),
    ('smosr_x2_dys_d16_m20_k3_n1_6x7', dict(dim=16, n_mb=1, upsampler='dysample', upsampler_mid_dim=20, d_kernel=3, head_gain=12.0), (2, 3, 6, 7), 1223),
]  # fmt: skip

_captured: dict = {}
# the registered loader's own globals (the registry imports the architecture packages by walking the file system, so the module object
# it holds need not be the one ``import`` returns)
_loader_globals = resselt.archs.internal_registry.get('SMoSR').load.__func__.__globals__
_RealSMoSR = _loader_globals['SMoSR']


def _capture(**kw):
    _captured.clear()
    _captured.update(kw)
    return _RealSMoSR(**kw)


_loader_globals['SMoSR'] = _pkg.SMoSR = _capture  # the loader's call site: what it inferred, as it hands it over
_RealSMoSR.forward.__globals__['torch'] = G._TorchNoPin()  # this family's own DySample asks for pinned memory too


def claims(sd) -> list:
    return [arch.id for arch in resselt.archs.internal_registry.store.values() if arch.detect(sd)]


def gate_stats(model, x) -> tuple[float, float]:
    """(median |g|, share of |g| > 3) over the gate pre-activations g of every SMB."""
    got, hooks = [], []
    for m in model.modules():
        if type(m).__name__ == 'SMB':
            hooks.append(m.body.register_forward_hook(lambda _m, _i, out: got.append(out.chunk(2, 1)[1].detach().abs().flatten())))
    with torch.no_grad():
        model(x.clone())
    for h in hooks:
        h.remove()
    g = torch.cat(got)
    return float(g.median()), float((g > 3).float().mean())


def main():
    for name, kw, shape, seed in CASES:
        sd = synth.smosr_state_dict(seed=seed, **kw)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'smosr.pth')
            torch.save(dict(sd), path)
            model = resselt.load_from_file(path).eval()
        hyper = {k: (v if isinstance(v, (str, float)) else int(v)) for k, v in _captured.items()}
        # the buffer a FRESHLY constructed reference module holds (load_state_dict overwrote the loaded one's with the checkpoint's)
        fresh_meta = [int(v) for v in _RealSMoSR(**_captured).upsampler.MetaUpsample]
        ref_sd = model.state_dict()
        assert list(ref_sd) == list(sd), name
        assert all(ref_sd[k].dtype == v.dtype and ref_sd[k].shape == v.shape for k, v in sd.items()), name
        # entering eval mode rewrites eval_conv.* from W / D / mul / bias: everything else is what was loaded
        assert all(torch.equal(ref_sd[k], v) for k, v in sd.items() if '.eval_conv.' not in k), name
        x = synth.synth_input(shape, seed)
        with torch.no_grad():
            y = model(x.clone())
            y64 = copy.deepcopy(model).double().eval()(x.double())
        median, above3 = gate_stats(model, x)
        who = claims(sd)
        meta = dict(arch='smosr', synth=kw, seed=seed, metadata=G.meta_of(model), hyper=hyper, claimed_by=who[0] if who else '', claims=who,
                    state_dict={k: list(v.shape) for k, v in ref_sd.items()}, dtypes={k: str(v.dtype) for k, v in ref_sd.items() if v.dtype != torch.float32},
                    meta_upsample=fresh_meta, y_absmax=float(y.abs().max()), f64_dev=float((y.double() - y64).abs().max()), gate_median=median, gate_above3=above3,
                    torch=torch.__version__, generator='tools/gen_golden_smosr.py')  # fmt: skip
        np.savez_compressed(os.path.join(G.OUT, name + '.npz'), meta=np.array(json.dumps(meta)), x=x.numpy(), y=y.numpy())
        size = os.path.getsize(os.path.join(G.OUT, name + '.npz'))
        print(f"{name}: x {tuple(x.shape)} -> y {tuple(y.shape)}  |y|max {meta['y_absmax']:.3f}  f32-f64 {meta['f64_dev']:.2e}  gate median {median:.3f}"
              f"  >3: {above3:.4f}  hyper {hyper}  {size} B")  # fmt: skip


if __name__ == '__main__':
    main()
