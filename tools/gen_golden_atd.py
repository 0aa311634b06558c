#!/usr/bin/env python3
"""Generate the ATD golden fixtures (tests/golden/atd_*.npz) by running the REAL reference in eval mode.

Imports tools/gen_golden.py for its import shims.  Writes only files with the prefix above.  Each fixture records the synthetic
checkpoint's arguments, the seed, the metadata the reference's loader inferred, the uid of the reference architecture that claimed the
state dict, the names and shapes of the reference module's state_dict (no weights) and, per layer, what AC_MSA did: the category ids
(``tk_id_<l>``), the permutation ``torch.sort(stable=False)`` returned (``perm_<l>``) and the smallest relative top-two margin of the
similarity map (``margins``).  ``y`` is the reference's output; ``y_stable`` its output with the sort made stable (the call is patched in
this process through the arch module's ``torch`` name, not in the reference tree) and ``tk_id_stable_<l>`` the ids of that run: the two
runs part after the first layer, so a free-running stable implementation follows the second one.  Outputs larger than 48 x 48 are cropped.

Guarded cases are chosen by seed search so that their smallest margin is at least TAU = 1e-4: on those the category decisions do not
depend on float rounding, and a free-running engine must reproduce ``tk_id`` and ``y_stable``.

Usage:  python tools/gen_golden_atd.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (applies the shims and imports the reference)

torch, resselt, synth = G.torch, G.resselt, G.synth
import resselt.archs.atd.arch as REF  # noqa: E402

CROP = 48
TAU = 1e-4

L48 = dict(embed_dim=48, depths=(2, 2), num_heads=(4, 4), window_size=8, num_tokens=64, reducted_dim=8, mlp_ratio=2.0)
CASES = [  # name, synth kwargs, input shape, first seed, guarded
    # light (category_size 128), n = 24 * 24 = 64 * 9: four and a half groups, the last one padded; head width 12
    ('atd_light_x2_w8_c48_24x24', dict(L48, upscale=2, upsampler='pixelshuffledirect'), (1, 3, 24, 24), 700, True),
    # the released classical shape at small depth: 210 / 6 heads = head width 35, window 16, 128 tokens, category_size 256, n = 1024 = 4 * 256
    ('atd_x4_c210_h6_w16_ps_20x27', dict(embed_dim=210, depths=(2,), num_heads=(6,), window_size=16, num_tokens=128, reducted_dim=10, mlp_ratio=2.0,
                                         upscale=4, upsampler='pixelshuffle'), (1, 3, 20, 27), 720, True),  # fmt: skip
    # denoising head, gray, batch 2, n = 256 = one whole group
    ('atd_x1_w8_c48_gray_b2_13x15', dict(L48, depths=(3,), num_heads=(4,), in_chans=1, upscale=1, upsampler=''), (2, 1, 13, 15), 740, True),
    # nearest+conv, 3conv, no_norm, a one-layer second block, n = 128 < category_size; head width 32
    ('atd_x4_w8_c64_nearest_3conv_nonorm_8x15', dict(embed_dim=64, depths=(2, 1), num_heads=(2, 2), window_size=8, num_tokens=64, reducted_dim=4,
                                                     mlp_ratio=2.0, upscale=4, upsampler='nearest+conv', resi_connection='3conv', norm=False),
     (1, 3, 8, 15), 760, True),  # fmt: skip
    # pixelshuffle x3, no qkv bias, n = 24 * 32 = 3 * 256 (not guarded: free-running parity is not asserted on it)
    ('atd_x3_w8_c48_ps_nobias_17x25', dict(L48, upscale=3, upsampler='pixelshuffle', qkv_bias=False), (1, 3, 17, 25), 780, False),
]


def claimed_by(sd) -> str:
    for arch in resselt.archs.internal_registry.store.values():
        if arch.detect(sd):
            return arch.id
    return ''


class TorchProxy:
    """Stands in for ``torch`` inside the reference's arch module: records what AC_MSA computes and can make its sort stable."""

    def __init__(self):
        self.stable = False
        self.records: list = []
        self.last_margin = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def argmax(self, sim, *a, **kw):
        t = sim.topk(2, dim=-1).values
        self.last_margin = float(((t[..., 0] - t[..., 1]) / t[..., 0]).min())
        return torch.argmax(sim, *a, **kw)

    def sort(self, x, *a, **kw):
        if self.stable:
            kw['stable'] = True
        out = torch.sort(x, *a, **kw)
        self.records.append((x.clone(), out[1].clone(), self.last_margin))
        return out


def run(model, x, proxy, stable):
    proxy.stable, proxy.records = stable, []
    with torch.no_grad():
        y = model(x.clone())
    return y, proxy.records


def save(name: str, meta: dict, **arrays):
    meta = dict(meta, torch=torch.__version__, generator='tools/gen_golden_atd.py')
    path = os.path.join(G.OUT, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f'{name}: {os.path.getsize(path)} bytes, seed {meta["seed"]}, min margin {meta["min_margin"]:.3e}, decisions {meta["decisions"]}')


def main():
    proxy = TorchProxy()
    REF.torch = proxy
    for name, kw, shape, seed0, guarded in CASES:
        for seed in range(seed0, seed0 + 20):
            sd = synth.atd_state_dict(seed=seed, **kw)
            model = resselt.load_from_state_dict(dict(sd)).eval()
            x = synth.synth_input(shape, seed)
            y, log = run(model, x, proxy, False)
            y_stable, log_s = run(model, x, proxy, True)
            margin = min(m for _, _, m in log + log_s)  # both trajectories: they part after the first layer
            if not guarded or margin >= TAU:
                break
            print(f'  {name}: seed {seed} has margin {margin:.3e} < {TAU}, next')
        else:
            raise SystemExit(f'{name}: no seed with a margin >= {TAU}')
        keys = {k: list(v.shape) for k, v in model.state_dict().items()}
        decisions = sum(int(i.numel()) for i, _, _ in log)
        meta = dict(arch='atd', synth={k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, seed=seed, metadata=G.meta_of(model),
                    claimed_by=claimed_by(sd), mode='eval', state_dict=keys, guarded=guarded, min_margin=margin, decisions=decisions, tau=TAU,
                    layers=len(log), category_size=model.layers[0].residual_group.layers[0].attn_aca.category_size)  # fmt: skip
        full = list(y.shape)
        crop = None
        if y.shape[2] > CROP or y.shape[3] > CROP:
            crop = [0, CROP, 0, CROP]
            y, y_stable = y[:, :, :CROP, :CROP], y_stable[:, :, :CROP, :CROP]
        arrays = dict(x=x, y=y, y_stable=y_stable, margins=np.array([m for _, _, m in log], dtype=np.float64))
        for li, (ids, perm, _) in enumerate(log):
            arrays[f'tk_id_{li}'] = ids.numpy().astype(np.int16)
            arrays[f'perm_{li}'] = perm.numpy().astype(np.int32)
            arrays[f'tk_id_stable_{li}'] = log_s[li][0].numpy().astype(np.int16)
        save(name, dict(meta, crop=crop, y_shape=full), **arrays)
    REF.torch = torch


if __name__ == '__main__':
    main()
