"""Plain-PyTorch restatements (in the dtype of the input: fp32, or fp64 for a high-precision reference) of the MoSR and MoSRv2 forwards from a state dict (CPU), written from the layer descriptions in
resselt_amd/archs/mosr and resselt_amd/archs/mosrv2.  ``mosrv2_forward`` also takes the x1 ``unshuffle_mod`` checkpoints the reference
loader reads wrongly."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _conv(sd, key, x, pad=None):
    w = sd[f'{key}.weight']
    return F.conv2d(x, w, sd[f'{key}.bias'], padding=w.shape[-1] // 2 if pad is None else pad)


def _layer_norm(x, w, b, eps=1e-6):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]


def _rms_norm(x, scale, offset, eps=1e-6):
    rms = x.norm(2, dim=1, keepdim=True) * x.shape[1] ** -0.5
    return scale * (x / (rms + eps)) + offset


def _dw(x, w, b):
    return F.conv2d(x, w, b, padding=(w.shape[2] // 2, w.shape[3] // 2), groups=w.shape[0])


def _gated(sd, b, x, hidden, conv_fn):
    f = _conv(sd, f'{b}.fc1', x)
    g, rest = f[:, :hidden], f[:, hidden:]
    return F.mish(_conv(sd, f'{b}.fc2', F.mish(g) * conv_fn(rest)))


def dysample(sd, key, x, scale, groups=4):
    """Learning to Upsample by Learning to Sample (arXiv 2308.15085) as the reference heads configure it, with the end 1x1 convolution."""
    B, _, H, W = x.shape
    off = F.conv2d(x, sd[f'{key}.offset.weight'], sd[f'{key}.offset.bias']) * torch.sigmoid(F.conv2d(x, sd[f'{key}.scope.weight'])) * 0.5
    off = (off + sd[f'{key}.init_pos']).view(B, 2, -1, H, W)
    cy, cx = torch.meshgrid(torch.arange(H, dtype=x.dtype) + 0.5, torch.arange(W, dtype=x.dtype) + 0.5, indexing='ij')
    base = torch.stack([cx, cy]).view(1, 2, 1, H, W)
    norm = torch.tensor([W, H], dtype=x.dtype).view(1, 2, 1, 1, 1)
    coords = 2 * (base + off) / norm - 1
    coords = F.pixel_shuffle(coords.reshape(B, -1, H, W), scale).view(B, 2, -1, scale * H, scale * W).permute(0, 2, 3, 4, 1).flatten(0, 1)
    out = F.grid_sample(x.reshape(B * groups, -1, H, W), coords, mode='bilinear', align_corners=False, padding_mode='border')
    out = out.view(B, -1, scale * H, scale * W)
    return F.conv2d(out, sd[f'{key}.end_conv.weight'], sd[f'{key}.end_conv.bias'])


def _trunk_tail(sd, t, x):
    x = F.mish(_conv(sd, f'gblocks.{t}', x))
    x = F.mish(_conv(sd, f'gblocks.{t + 2}', x))
    return _conv(sd, f'gblocks.{t + 4}', x)


def mosr_forward(sd, x, upsampler, upscale):
    sd = {k: v.to(x.dtype) for k, v in sd.items()}
    n_block = 0
    while f'gblocks.{n_block + 1}.fc1.weight' in sd:
        n_block += 1
    h = _conv(sd, 'gblocks.0', x)
    for i in range(1, n_block + 1):
        b = f'gblocks.{i}'
        hidden = sd[f'{b}.fc2.weight'].shape[1]
        cc = sd[f'{b}.conv.weight'].shape[0]

        def conv_fn(rest, b=b, hidden=hidden, cc=cc):
            return torch.cat([rest[:, : hidden - cc], _dw(rest[:, hidden - cc :], sd[f'{b}.conv.weight'], sd[f'{b}.conv.bias'])], 1)

        h = _gated(sd, b, _layer_norm(h, sd[f'{b}.norm.weight'], sd[f'{b}.norm.bias']), hidden, conv_fn) + (h - 0.5)
    h = _trunk_tail(sd, n_block + 1, h)
    sc = F.mish(_conv(sd, 'shortcut.block.2', F.mish(_conv(sd, 'shortcut.block.0', x)))) + _conv(sd, 'shortcut.conv11', x)
    h = h + (sc - 0.5)
    if upsampler == 'ps':
        return F.pixel_shuffle(_conv(sd, 'upsampler.0', h), upscale)
    if upsampler == 'gps':
        y = _conv(sd, 'upsampler.in_to_k', h)
        y = y.reshape(y.shape[0], 8, -1, *y.shape[-2:]).mean(1)
        return F.pixel_shuffle(y, upscale)
    return dysample(sd, 'upsampler', h, upscale)


def mosrv2_forward(sd, x, upsampler, scale, mid_dim=32):
    """``scale``: the model's scale (the output is scale x the input); ``unshuffle_mod`` is read from the keys."""
    sd = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith('MetaUpsample')}
    unshuffle = 'gblocks.1.weight' in sd and 'gblocks.0.weight' not in sd
    u, s_int, first = (4 // scale, 4, 2) if unshuffle else (1, scale, 1)
    _, _, h, w = x.shape
    ph, pw = (u - h % u) % u, (u - w % u) % u
    xp = F.pad(x, (0, pw, 0, ph), 'reflect') if (ph or pw) else x
    f = F.pixel_unshuffle(xp, u) if u > 1 else xp
    t = _conv(sd, f'gblocks.{first - 1}', f)
    i = first
    while f'gblocks.{i}.fc1.weight' in sd:
        b = f'gblocks.{i}'
        dim = t.shape[1]
        hidden = sd[f'{b}.fc2.weight'].shape[1]
        gc = sd[f'{b}.conv.dwconv_hw.weight'].shape[0]
        if f'{b}.norm.scale' in sd:
            n = _rms_norm(t, sd[f'{b}.norm.scale'], sd[f'{b}.norm.offset'])
        else:
            n = _layer_norm(t, sd[f'{b}.norm.weight'], sd[f'{b}.norm.bias'])

        def conv_fn(rest, b=b, hidden=hidden, dim=dim, gc=gc):
            i_id = hidden - 3 * gc
            parts = [rest[:, :i_id]]
            for j, name in enumerate(('dwconv_hw', 'dwconv_w', 'dwconv_h')):
                parts.append(_dw(rest[:, i_id + j * gc : i_id + (j + 1) * gc], sd[f'{b}.conv.{name}.weight'], sd[f'{b}.conv.{name}.bias']))
            return torch.cat(parts, 1)

        t = _gated(sd, b, n, hidden, conv_fn) * sd[f'{b}.gamma'] + t
        i += 1
    t = _trunk_tail(sd, i, t)
    y = _head(sd, t, upsampler, s_int, mid_dim)
    y = y + F.interpolate(xp, scale_factor=scale, mode='bilinear', align_corners=False)
    return y[:, :, : h * scale, : w * scale]


def _head(sd, t, up, s, mid_dim):
    lrelu = F.leaky_relu
    if s == 1 or up == 'conv':
        return _conv(sd, 'to_img.0', t)
    if up == 'pixelshuffledirect':
        return F.pixel_shuffle(_conv(sd, 'to_img.0', t), s)
    if up == 'pixelshuffle':
        y, i = lrelu(_conv(sd, 'to_img.0', t), 0.01), 2
        for r in [2] * int(math.log2(s)) if s & (s - 1) == 0 else [3]:
            y = F.pixel_shuffle(_conv(sd, f'to_img.{i}', y), r)
            i += 2
        return _conv(sd, f'to_img.{i}', y)
    if up == 'nearest+conv':
        y, i = t, 0
        for r in [2] * int(math.log2(s)) if s & (s - 1) == 0 else [3]:
            y = lrelu(F.interpolate(_conv(sd, f'to_img.{i}', y), scale_factor=r, mode='nearest'), 0.2)
            i += 3
        y = lrelu(_conv(sd, f'to_img.{i}', y), 0.2)
        return _conv(sd, f'to_img.{i + 2}', y)
    if 'to_img.0.weight' in sd:
        return dysample(sd, 'to_img.2', lrelu(_conv(sd, 'to_img.0', t), 0.01), s)
    return dysample(sd, 'to_img.0', t, s)
