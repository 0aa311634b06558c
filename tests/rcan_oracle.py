"""Plain-torch CPU restatement of RCAN's forward pass (reference archs/rcan/arch.py:320-332) on a state dict, in the dtype of its input, written from the
module's structure: it is what the GPU tests compare larger inputs with, and tests/test_rcan_oracle.py pins it to the reference's own
outputs.  Unlike the reference it leaves its input alone."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _conv(sd, name, x):
    w = sd[f'{name}.weight']
    return F.conv2d(x, w, sd[f'{name}.bias'], padding=w.shape[-1] // 2)


def rcan_hyper(sd) -> dict:
    """What the loader reads off the keys."""
    groups = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('body.')) - 1
    blocks = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('body.0.body.')) - 1
    unshuffle = 'head.1.weight' in sd
    n_colors = sd['tail.1.weight'].shape[0]
    down = int(math.sqrt(sd['head.1.weight'].shape[1] / n_colors)) if unshuffle else 1
    ups = sorted(int(k.split('.')[2]) for k in sd if k.startswith('tail.0.') and k.endswith('.weight'))
    return dict(groups=groups, blocks=blocks, down=down, ups=ups, norm='sub_mean.weight' in sd)


def rcan_forward(sd, x: torch.Tensor) -> torch.Tensor:
    sd = {k: v.to(x.dtype) for k, v in sd.items()}
    hp = rcan_hyper(sd)
    _, _, h, w = x.shape
    d = hp['down']
    x = F.pad(x, (0, (d - w % d) % d, 0, (d - h % d) % d), 'reflect')
    rng = 255.0 if hp['norm'] else 1.0
    x = x * rng
    if hp['norm']:
        x = _conv(sd, 'sub_mean', x)
    if d > 1:
        x = _conv(sd, 'head.1', F.pixel_unshuffle(x, d))
    else:
        x = _conv(sd, 'head.0', x)
    res = x
    for g in range(hp['groups']):
        gin = res
        for b in range(hp['blocks']):
            p = f'body.{g}.body.{b}.body'
            t = _conv(sd, f'{p}.2', F.relu(_conv(sd, f'{p}.0', res)))
            m = t.mean(dim=(2, 3), keepdim=True)
            gate = torch.sigmoid(_conv(sd, f'{p}.3.conv_du.2', F.relu(_conv(sd, f'{p}.3.conv_du.0', m))))
            res = t * gate + res
        res = _conv(sd, f'body.{g}.body.{hp["blocks"]}', res) + gin
    res = _conv(sd, f'body.{hp["groups"]}', res) + x
    scale = 1
    for i in hp['ups']:
        res = _conv(sd, f'tail.0.{i}', res)
        r = math.isqrt(res.shape[1] // sd['tail.1.weight'].shape[1])
        res = F.pixel_shuffle(res, r)
        scale *= r
    y = _conv(sd, 'tail.1', res)
    if hp['norm']:
        y = _conv(sd, 'add_mean', y)
    out = scale // d
    return (y / rng)[:, :, : h * out, : w * out]
