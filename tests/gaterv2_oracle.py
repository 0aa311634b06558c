"""Plain-PyTorch restatement (in the dtype of the input: fp64 for a high-precision reference) of the GateRv2 forward from a state dict (CPU),
written from the layer description in resselt_amd/archs/gaterv2.  The MetaGated blocks are tests/gaterv3_oracle.py's (the two families
share them); the latent token mixer, the ConvBlock shortcut and the output are GateRv2's own.  The query / key / value convolutions are
applied one by one in the reference's channel order (the engine runs them as one padded convolution).  Above x1 the output is the FULL
``H scale x W scale`` image (a 'conv' head does not upsample: the padded map cropped to at most that), as the engine returns it.  It raises
where the reference raises: the reflect pad of a side that is too small, and a decoder with fewer levels than the encoder."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from gaterv3_oracle import _conv, _count, _rms, meta_gated
from gfisrv2_oracle import head

MODES = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')
EPS = 1e-6


def linear_attention(q, k, v, eps=EPS):
    """q, k [B, m, N], v [B, C, N] -> [B, C, N]: q and k scaled to unit l2 norm per token (no epsilon), then
    out[c, n] = (sum_n' v[c, n'] + sum_j q[j, n] sum_n' k[j, n'] v[c, n']) / (N + sum_j q[j, n] (sum_n' k[j, n'] + eps))."""
    n = q.shape[2]
    q = q * (1 / q.norm(dim=1, keepdim=True))
    k = k * (1 / k.norm(dim=1, keepdim=True))
    ksum = k.sum(2) + eps  # [B, m]
    vsum = v.sum(2)  # [B, C]
    mat = k @ v.transpose(1, 2)  # [B, m, C]
    t = 1 / (n + (q * ksum[:, :, None]).sum(1))  # [B, N]
    return (vsum[:, :, None] + mat.transpose(1, 2) @ q) * t[:, None, :]


def attention(sd, p, x):
    b, c, h, w = x.shape
    q, k, v = (_conv(sd, f'{p}.{name}', x).reshape(b, -1, h * w) for name in ('query_conv', 'key_conv', 'value_conv'))
    return linear_attention(q, k, v).reshape(b, c, h, w)


def latent_block(sd, b, x):
    w, hidden = x.shape[1], sd[f'{b}.fc2.weight'].shape[1]
    g, i, c = torch.split(_conv(sd, f'{b}.fc1', _rms(sd, f'{b}.norm', x)), [hidden, hidden - w, w], 1)
    return F.mish(_conv(sd, f'{b}.fc2', F.mish(g) * torch.cat([i, attention(sd, f'{b}.token_mix', c)], 1)))


def gaterv2_forward(sd, x):
    """``sd``: a GateRv2 state dict (``upsample.MetaUpsample`` names the head and the scale; none: x1); ``x`` [N, C, H, W]."""
    scale, mode = 1, 'conv'
    if 'upsample.MetaUpsample' in sd:
        _, index, scale = (int(v) for v in sd['upsample.MetaUpsample'][:3])
        mode = MODES[index]
    sd = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith('MetaUpsample')}
    levels = _count(sd, 'encode')
    P = 1 << levels
    H, W = x.shape[-2:]
    inp = F.pad(x, (0, (P - W % P) % P, 0, (P - H % P) % P), 'reflect')
    t = _conv(sd, 'in_to_dim', inp)
    shorts = []
    for j in range(levels):
        for i in range(_count(sd, f'encode.{j}.gated')):
            t = meta_gated(sd, f'encode.{j}.gated.{i}', t)
        shorts.append(t)
        t = F.pixel_unshuffle(_conv(sd, f'encode.{j}.scale.0', t), 2)
    for i in range(_count(sd, 'latent')):
        t = latent_block(sd, f'latent.{i}', t)
    shorts.reverse()
    for i in range(_count(sd, 'decode')):
        t = torch.cat([F.pixel_shuffle(_conv(sd, f'decode.{i}.scale.0', t), 2), shorts[i]], 1)
        t = _conv(sd, f'decode.{i}.shor', t)
        for k in range(_count(sd, f'decode.{i}.gated')):
            t = meta_gated(sd, f'decode.{i}.gated.{k}', t)
    if scale == 1:
        return (_conv(sd, 'dim_to_in', t) + inp)[:, :, :H, :W]
    s = 'short_to_dim'
    block = F.mish(_conv(sd, f'{s}.block.2', F.mish(_conv(sd, f'{s}.block.0', inp))))
    t = t + block + _conv(sd, f'{s}.conv11', inp)
    y = head({k.replace('upsample.', 'upscale.'): v for k, v in sd.items()}, t, mode, scale)
    return y[:, :, : H * scale, : W * scale]
