"""Plain-PyTorch restatement (in the dtype of the input: fp64 for a high-precision reference) of the GateRV3 forward from a state dict (CPU),
written from the layer description in resselt_amd/archs/gaterv3.  Independent of the engine where the engine transforms weights: every
Conv3XC is computed UNFOLDED, as 1x1 -> 3x3 (valid) -> 1x1 on the zero-padded input plus the 1x1 skip (the stored ``eval_conv.*`` tensors
are ignored, as ``conv.*`` / ``sk`` win over them); fc1 / fc2 are used in the reference's channel order; the attention normalises q and k
before the product.  It raises where the reference raises: the reflect pad of a side that is too small, and a decoder with fewer levels than
the encoder (a channel mismatch in the first convolution that meets it)."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from gfisrv2_oracle import head

MODES = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')
HEADS = 16


def _conv(sd, key, x):
    w = sd[f'{key}.weight']
    return F.conv2d(x, w, sd.get(f'{key}.bias'), padding=w.shape[-1] // 2)


def _dw(sd, key, x):
    w = sd[f'{key}.weight']
    return F.conv2d(x, w, sd[f'{key}.bias'], padding=(w.shape[2] // 2, w.shape[3] // 2), groups=w.shape[0])


def _rms(sd, key, x, eps=1e-6):
    rms = x.norm(2, dim=1, keepdim=True) * x.shape[1] ** -0.5
    return sd[f'{key}.scale'][:, None, None] * (x / (rms + eps)) + sd[f'{key}.offset'][:, None, None]


def conv3xc(sd, p, x):
    y = F.conv2d(F.pad(x, (1, 1, 1, 1)), sd[f'{p}.conv.0.weight'], sd.get(f'{p}.conv.0.bias'))
    y = F.conv2d(y, sd[f'{p}.conv.1.weight'], sd.get(f'{p}.conv.1.bias'))
    y = F.conv2d(y, sd[f'{p}.conv.2.weight'], sd.get(f'{p}.conv.2.bias'))
    return y + F.conv2d(x, sd[f'{p}.sk.weight'], sd.get(f'{p}.sk.bias'))


def spab(sd, p, x):
    o1 = F.silu(conv3xc(sd, f'{p}.c1_r', x))
    o3 = conv3xc(sd, f'{p}.c3_r', F.silu(conv3xc(sd, f'{p}.c2_r', o1)))
    return (o3 + x) * (torch.sigmoid(o3) - 0.5), o1


def attention(sd, p, x):
    b, c, h, w = x.shape
    q, k, v = (t.reshape(b, HEADS, c // HEADS, h * w) for t in _dw(sd, f'{p}.qkv_dwconv', _conv(sd, f'{p}.qkv', x)).chunk(3, 1))
    q = q / q.norm(dim=3, keepdim=True).clamp_min(1e-12)
    k = k / k.norm(dim=3, keepdim=True).clamp_min(1e-12)
    a = torch.softmax(q @ k.transpose(2, 3) * sd[f'{p}.temperature'], 3)
    return _conv(sd, f'{p}.project_out', (a @ v).reshape(b, c, h, w))


def gated_cnn(sd, b, x):
    w, hidden = x.shape[1], sd[f'{b}.fc2.weight'].shape[1]
    g, i, c = torch.split(_conv(sd, f'{b}.fc1', _rms(sd, f'{b}.norm', x)), [hidden, hidden - w, w], 1)
    if f'{b}.token_mix.qkv.weight' in sd:
        c = attention(sd, f'{b}.token_mix', c)
    else:
        gc = int(w * 0.125)
        c_id, c_hw, c_w, c_h = torch.split(c, [w - 3 * gc, gc, gc, gc], 1)
        c = torch.cat([c_id, _dw(sd, f'{b}.token_mix.dwconv_hw', c_hw), _dw(sd, f'{b}.token_mix.dwconv_w', c_w), _dw(sd, f'{b}.token_mix.dwconv_h', c_h)], 1)
    return F.mish(_conv(sd, f'{b}.fc2', F.mish(g) * torch.cat([i, c], 1)))


def meta_gated(sd, b, x):
    w = x.shape[1]
    t = _conv(sd, f'{b}.local.1', _rms(sd, f'{b}.local.0', x))
    t = F.conv2d(t, sd[f'{b}.local.2.weight'], sd[f'{b}.local.2.bias'], padding=1, groups=w)
    s = t[:, :w] * t[:, w:]
    x = s * _conv(sd, f'{b}.sca.1', s.mean((2, 3), keepdim=True)) * sd[f'{b}.gamma0'] + x
    return gated_cnn(sd, f'{b}.glob', x) * sd[f'{b}.gamma1'] + x


def _count(sd, prefix):
    n = 0
    while any(k.startswith(f'{prefix}.{n}.') for k in sd):
        n += 1
    return n


def gaterv3_forward(sd, x):
    """``sd``: a GateRV3 state dict (``dim_to_in.MetaUpsample`` names the head and the scale; none: x1); ``x`` [N, C, H, W]."""
    scale, mode = 1, 'conv'
    if 'dim_to_in.MetaUpsample' in sd:
        _, index, scale = (int(v) for v in sd['dim_to_in.MetaUpsample'][:3])
        mode = MODES[index]
    sd = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith('MetaUpsample')}
    levels = _count(sd, 'gater_encode')
    P = 1 << levels
    H, W = x.shape[-2:]
    inp = F.pad(x, (0, (P - W % P) % P, 0, (P - H % P) % P), 'reflect')
    t = _conv(sd, 'in_to_dim', inp)
    sisr, _ = spab(sd, 'span_block0', t)
    sisr_short = sisr
    for i in range(_count(sd, 'span_n_b')):
        sisr, _ = spab(sd, f'span_n_b.{i}', sisr)
    sisr, sisr_out = spab(sd, 'span_end', sisr)
    sisr = _conv(sd, 'sisr_cat_conv', torch.cat([t, conv3xc(sd, 'sisr_end_conv', sisr), sisr_short, sisr_out], 1))
    shorts = []
    for j in range(levels):
        for i in range(_count(sd, f'gater_encode.{j}.gated')):
            t = meta_gated(sd, f'gater_encode.{j}.gated.{i}', t)
        shorts.append(t)
        t = F.pixel_unshuffle(_conv(sd, f'gater_encode.{j}.scale.0', t), 2)
    for i in range(_count(sd, 'latent')):
        t = gated_cnn(sd, f'latent.{i}', t)
    shorts.reverse()
    for i in range(_count(sd, 'decode')):
        t = torch.cat([F.pixel_shuffle(_conv(sd, f'decode.{i}.scale.0', t), 2), shorts[i]], 1)
        t = _conv(sd, f'decode.{i}.shor', t)
        for k in range(_count(sd, f'decode.{i}.gated')):
            t = meta_gated(sd, f'decode.{i}.gated.{k}', t)
    t = t + sisr
    if scale == 1:
        y = _conv(sd, 'dim_to_in', t)
        up = inp
    else:
        y = head({k.replace('dim_to_in.', 'upscale.'): v for k, v in sd.items()}, t, mode, scale)
        up = F.interpolate(inp, scale_factor=scale, mode='nearest')
    gamma = sd['gamma'] if 'gamma' in sd else torch.ones(1, x.shape[1], 1, 1, dtype=x.dtype)
    return (y + gamma * up)[:, :, : H * scale, : W * scale]
