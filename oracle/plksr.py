"""Oracle for PLKSR and RealPLKSR (TEST INFRASTRUCTURE, see oracle/__init__.py).

Functional fp32 restatement of ``resselt/archs/plksr/plksr.py`` and ``rplksr.py`` in eval mode over the checkpoint's own key names.  The
sparse large-kernel layers run UNFOLDED, as the reference's forward does: SparsePLK as four dilated 5x5 convolutions summed,
RectSparsePLK as its m x n, n x m and n x n convolutions summed -- never as the one dense kernel the engine folds them into at pack time.
Pinned by tests/golden/plksr_*.npz and realplksr_*.npz (outputs of the reference itself).
"""

from __future__ import annotations

from typing import Mapping

import torch
import torch.nn.functional as F

from .span import dysample

# the reference loader's fixed SparsePLK sub-kernels: 5 x 5 at dilations 1..4, no max kernel, no identity (plksr/__init__.py:57-61)
SPARSE_DILATIONS = (1, 2, 3, 4)
NORM_GROUPS = 4  # plksr/__init__.py:116


def _seq_len(sd, prefix: str) -> int:
    idx = {int(k[len(prefix) + 1 :].split('.')[0]) for k in sd if k.startswith(prefix + '.')}
    return max(idx) + 1


def _conv(sd, key, x, padding='same', dilation=1):
    return F.conv2d(x, sd[f'{key}.weight'], sd[f'{key}.bias'], padding=padding, dilation=dilation)


def large_kernel(sd, key, x):
    """PLKConv2d (plksr.py:65-81, rplksr.py:31-37; with_idt off), SparsePLKConv2d (plksr.py:155-166) or RectSparsePLKConv2d
    (plksr.py:112-119) on the first pdim channels; the rest pass through."""
    if f'{key}.conv.weight' in sd:
        w = sd[f'{key}.conv.weight']
        pdim, k = w.shape[0], w.shape[2]
        y = _conv(sd, f'{key}.conv', x[:, :pdim], padding=k // 2)
    elif f'{key}.convs.0.weight' in sd:
        pdim = sd[f'{key}.convs.0.weight'].shape[0]
        x1 = x[:, :pdim]
        y = 0.0
        for j, d in enumerate(SPARSE_DILATIONS):
            ks = sd[f'{key}.convs.{j}.weight'].shape[2]
            y = y + _conv(sd, f'{key}.convs.{j}', x1, padding=(ks // 2) * d, dilation=d)
    else:
        pdim = sd[f'{key}.mn_conv.weight'].shape[0]
        x1 = x[:, :pdim]
        y = 0.0
        for name in ('mn_conv', 'nm_conv', 'nn_conv'):
            kh, kw = sd[f'{key}.{name}.weight'].shape[2:]
            y = y + _conv(sd, f'{key}.{name}', x1, padding=(kh // 2, kw // 2))
    return torch.cat([y, x[:, pdim:]], dim=1)


def plk_block(sd, key, x, real):
    """PLKBlock.forward (plksr.py:317-323; rplksr.py:85-93 adds GroupNorm(4) before the skip, and its mixer is always DCCM with Mish)."""
    mixer = f'{key}.channel_mixer' if real else f'{key}.channe_mixer'
    act = F.mish if real else F.gelu  # nn.Mish (rplksr.py:16), exact nn.GELU (plksr.py:24, 36, 48)
    y = _conv(sd, f'{mixer}.2', act(_conv(sd, f'{mixer}.0', x)))
    y = large_kernel(sd, f'{key}.lk', y)
    if f'{key}.attn.f.0.weight' in sd:
        y = y * torch.sigmoid(_conv(sd, f'{key}.attn.f.0', y))  # EA (plksr.py:255-256)
    y = _conv(sd, f'{key}.refine', y)
    if real:
        y = F.group_norm(y, NORM_GROUPS, sd[f'{key}.norm.weight'], sd[f'{key}.norm.bias'])
    return y + x


def plksr_forward(sd: Mapping[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """plksr.forward (plksr.py:374-377) and realplksr.forward (rplksr.py:145-147); Dropout2d is the identity in eval mode."""
    real = 'feats.1.channel_mixer.0.weight' in sd
    n_feats = _seq_len(sd, 'feats')
    n_blocks = n_feats - (3 if real else 2)
    c = x.shape[1]
    last = sd[f'feats.{n_feats - 1}.weight']
    scale = round((last.shape[0] // c) ** 0.5)
    y = _conv(sd, 'feats.0', x)
    for b in range(1, n_blocks + 1):
        y = plk_block(sd, f'feats.{b}', y, real)
    y = _conv(sd, f'feats.{n_feats - 1}', y) + torch.repeat_interleave(x, scale * scale, dim=1)
    if 'to_img.init_pos' not in sd:
        return F.pixel_shuffle(y, scale)
    # DySample head (rplksr.py:133-141): groups = out_ch for an odd scale, else 4; no end convolution at x1 -- an identity 1x1 then
    groups = c if scale % 2 else 4
    if 'to_img.end_conv.weight' not in sd:
        cin = y.shape[1]
        sd = dict(sd, **{'to_img.end_conv.weight': torch.eye(cin, dtype=y.dtype, device=y.device)[:, :, None, None],
                         'to_img.end_conv.bias': torch.zeros(cin, dtype=y.dtype, device=y.device)})  # fmt: skip
    return dysample(sd, 'to_img', y, scale, groups)
