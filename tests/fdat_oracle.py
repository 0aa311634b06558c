"""Plain-torch FDAT forward (reference ``resselt/archs/fdat/arch.py``, eval mode) from a state dict: the CPU oracle of the FDAT tests.

It does not import the reference.  Hyper-parameters are read from the state dict the way the loader reads them (fdat/__init__.py).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')


def _conv(sd, name, x, pad=None):
    w = sd[f'{name}.weight']
    return F.conv2d(x, w, sd.get(f'{name}.bias'), padding=w.shape[-1] // 2 if pad is None else pad)


def _lin(sd, name, x):
    return F.linear(x, sd[f'{name}.weight'], sd.get(f'{name}.bias'))


def _spatial_attention(sd, a, x, H, W, heads, ws):
    B, L, C = x.shape
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(x.view(B, H, W, C), (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = H + pad_b, W + pad_r
    x = x.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    q, k, v = _lin(sd, f'{a}.qkv', x).view(-1, ws * ws, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    attn = (q * (C // heads) ** -0.5) @ k.transpose(-2, -1) + sd[f'{a}.bias']
    x = (attn.softmax(-1) @ v).transpose(1, 2).reshape(-1, ws * ws, C)
    x = _lin(sd, f'{a}.proj', x).view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    return x[:, :H, :W].reshape(B, L, C)


def _channel_attention(sd, a, x, heads):
    B, N, C = x.shape
    q, k, v = _lin(sd, f'{a}.qkv', x).view(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k = F.normalize(q.transpose(-2, -1), dim=-1), F.normalize(k.transpose(-2, -1), dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * sd[f'{a}.temp']).softmax(-1)
    return _lin(sd, f'{a}.proj', (attn @ v.transpose(-2, -1)).permute(0, 3, 1, 2).reshape(B, N, C))


def _block(sd, b, x, H, W, spatial, heads, ws):
    B, L, C = x.shape
    g = lambda t: t.transpose(1, 2).reshape(B, -1, H, W)  # noqa: E731  tokens -> map
    t = lambda m: m.reshape(B, m.shape[1], L).transpose(1, 2)  # noqa: E731  map -> tokens
    n1 = F.layer_norm(x, (C,), sd[f'{b}.n1.weight'], sd[f'{b}.n1.bias'], 1e-5)
    a = _spatial_attention(sd, f'{b}.attn', n1, H, W, heads, ws) if spatial else _channel_attention(sd, f'{b}.attn', n1, heads)
    c = t(F.gelu(F.conv2d(g(n1), sd[f'{b}.conv.0.weight'], padding=1, groups=C)))
    if spatial:  # channel_modulates_spatial: the channel gate of the conv branch scales the attention output
        m = g(c).mean((2, 3), keepdim=True)
        cm = torch.sigmoid(F.conv2d(F.gelu(F.conv2d(m, sd[f'{b}.inter.cg.1.weight'])), sd[f'{b}.inter.cg.3.weight']))
        f = a * cm.view(B, 1, C) + c
    else:  # spatial_modulates_channel
        f = a + c * torch.sigmoid(t(F.conv2d(g(a), sd[f'{b}.inter.sg.0.weight'])))
    x = x + f
    n2 = F.layer_norm(x, (C,), sd[f'{b}.n2.weight'], sd[f'{b}.n2.bias'], 1e-5)
    h = F.gelu(_lin(sd, f'{b}.ffn.fc1', n2))
    h = t(F.conv2d(g(h), sd[f'{b}.ffn.smix.weight'], padding=1, groups=h.shape[-1]))
    return x + _lin(sd, f'{b}.ffn.fc2', h)


def _dysample(sd, d, x, scale, groups=4):
    offset = _conv(sd, f'{d}.offset', x) * torch.sigmoid(_conv(sd, f'{d}.scope', x)) * 0.5 + sd[f'{d}.init_pos']
    B, _, H, W = offset.shape
    offset = offset.view(B, 2, -1, H, W)
    coords = torch.stack(torch.meshgrid([torch.arange(W, dtype=x.dtype, device=x.device) + 0.5, torch.arange(H, dtype=x.dtype, device=x.device) + 0.5], indexing='ij')).transpose(1, 2).unsqueeze(1).unsqueeze(0)
    coords = 2 * (coords + offset) / torch.tensor([W, H], dtype=x.dtype, device=x.device).view(1, 2, 1, 1, 1) - 1
    coords = F.pixel_shuffle(coords.reshape(B, -1, H, W), scale).view(B, 2, -1, scale * H, scale * W).permute(0, 2, 3, 4, 1).contiguous().flatten(0, 1)
    out = F.grid_sample(x.reshape(B * groups, -1, H, W), coords, mode='bilinear', align_corners=False, padding_mode='border')
    return _conv(sd, f'{d}.end_conv', out.view(B, -1, scale * H, scale * W))


def _channel_ln(x, w, b, eps=1e-6):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]


def _lda(sd, u, x, scale, groups=2, rng=11.0):
    B, C, H, W = x.shape
    Ho, Wo = H * scale, W * scale
    hid = C // 4
    n = _channel_ln(x, sd[f'{u}.layer_norm.weight'], sd[f'{u}.layer_norm.bias'])
    q = F.interpolate(F.conv2d(n, sd[f'{u}.proj_q.weight']), (Ho, Wo), mode='bilinear', align_corners=True)
    k = F.conv2d(n, sd[f'{u}.proj_k.weight'])
    gc = hid // groups
    o = F.conv2d(q.view(B * groups, gc, Ho, Wo), sd[f'{u}.conv_offset.0.weight'], padding=1, groups=gc)
    o = F.silu(_channel_ln(o, sd[f'{u}.conv_offset.1.weight'], sd[f'{u}.conv_offset.1.bias']))
    o = _conv(sd, f'{u}.conv_offset.3', o)
    base = torch.arange(-1, 2, dtype=x.dtype, device=x.device)
    base_off = torch.stack([base.repeat_interleave(3), base.repeat(3)], 1).flatten().view(1, -1, 1, 1)
    o = (o.tanh() * rng + base_off).view(B * groups, 3, 3, 2, Ho, Wo).permute(0, 1, 4, 2, 5, 3)  # b kh h kw w d
    rows, cols = torch.meshgrid(torch.arange(Ho, device=x.device), torch.arange(Wo, device=x.device), indexing='ij')
    o = (o + torch.stack((rows, cols), -1).view(1, 1, Ho, 1, Wo, 2)).contiguous().view(B * groups, 3 * Ho, 3 * Wo, 2)
    grid = torch.stack([2 * o[..., 1] / (Wo - 1) - 1, 2 * o[..., 0] / (Ho - 1) - 1], -1)

    def feats(t):
        s = F.grid_sample(t, grid, mode='bilinear', padding_mode='zeros', align_corners=True)  # (b g) c (kh h) (kw w)
        return s.view(B, groups, -1, 3, Ho, 3, Wo).permute(0, 4, 6, 3, 5, 1, 2).reshape(B, Ho * Wo, 9, -1)  # b (h w) (kh kw) (g c)

    ks = feats(k.reshape(B * groups, gc, H, W)) + sd[f'{u}.relative_position_bias_table'].view(1, 1, 9, hid)
    vs = feats(x.reshape(B * groups, C // groups, H, W))
    qh = q.permute(0, 2, 3, 1).reshape(B, Ho * Wo, 1, hid) * hid**-0.5
    return ((qh @ ks.transpose(-1, -2)).softmax(-1) @ vs).view(B, Ho, Wo, C).permute(0, 3, 1, 2)


def _upsampler(sd, x, mode, scale, dim, out, mid):
    up = 'upsampler'
    lrelu = lambda t, s: F.leaky_relu(t, s)  # noqa: E731
    pow2 = scale & (scale - 1) == 0
    if scale == 1 or mode == 'conv':
        return _conv(sd, f'{up}.0', x)
    if mode == 'pixelshuffledirect':
        return F.pixel_shuffle(_conv(sd, f'{up}.0', x), scale)
    if mode == 'pixelshuffle':
        x, i = lrelu(_conv(sd, f'{up}.0', x), 0.01), 2
        for r in [2] * int(math.log2(scale)) if pow2 else [3]:
            x, i = F.pixel_shuffle(_conv(sd, f'{up}.{i}', x), r), i + 2
        return _conv(sd, f'{up}.{i}', x)
    if mode == 'nearest+conv':
        i = 0
        for r in [2] * int(math.log2(scale)) if pow2 else [3]:
            x, i = lrelu(F.interpolate(_conv(sd, f'{up}.{i}', x), scale_factor=r), 0.2), i + 3
        return _conv(sd, f'{up}.{i + 2}', lrelu(_conv(sd, f'{up}.{i}', x), 0.2))
    if mode in ('dysample', 'lda'):
        i = 0
        if mid != dim:
            x, i = lrelu(_conv(sd, f'{up}.0', x), 0.01), 2
        if mode == 'dysample':
            return _dysample(sd, f'{up}.{i}', x, scale)
        return _conv(sd, f'{up}.{i + 1}', _lda(sd, f'{up}.{i}', x, scale))
    if mode == 'transpose+conv':
        def deconv(name, t):
            w = sd[f'{name}.weight']
            k = w.shape[-1]
            return F.conv_transpose2d(t, w, sd[f'{name}.bias'], stride=2 if k == 4 else 3, padding=1 if k == 4 else 0)

        if scale == 4:
            return _conv(sd, f'{up}.3', deconv(f'{up}.2', F.gelu(deconv(f'{up}.0', x))))
        return _conv(sd, f'{up}.1', deconv(f'{up}.0', x))
    # pa_up
    i = 0
    for r in [2] * int(math.log2(scale)) if pow2 else [3]:
        x = _conv(sd, f'{up}.{i + 1}', F.interpolate(x, scale_factor=r))
        x = lrelu(x * torch.sigmoid(_conv(sd, f'{up}.{i + 2}.conv.0', x)), 0.2)
        x, i = lrelu(_conv(sd, f'{up}.{i + 4}', x), 0.2), i + 6
    return _conv(sd, f'{up}.{i}', x)


def fdat_forward(sd, x):
    """The reference FDAT's eval forward for the checkpoint ``sd`` on ``x`` [N, C, h, w], in the dtype of ``x``."""
    sd = {k: v.to(x.dtype) if v.is_floating_point() else v for k, v in sd.items()}
    _, mi, scale, dim, out, mid, _ = [int(v) for v in sd['upsampler.MetaUpsample'].tolist()]
    mode = MODS[mi]
    bias = sd['groups.0.blocks.0.attn.bias']
    heads, ws = bias.shape[0], math.isqrt(bias.shape[2])
    n_groups = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('groups.'))
    n_blocks = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('groups.0.blocks.'))
    _, _, h, w = x.shape
    report = scale
    if 'conv_first.1.weight' in sd:  # unshuffle_mod: the module runs at scale 4 and reports 4 // factor
        u = math.isqrt(sd['conv_first.1.weight'].shape[1] // out)
        report = 4 // u
        x = F.pad(x, (0, (u - w % u) % u, 0, (u - h % u) % u), 'reflect')
        shallow = _conv(sd, 'conv_first.1', F.pixel_unshuffle(x, u))
    else:
        shallow = _conv(sd, 'conv_first', x)
    B, C, H, W = shallow.shape
    feat = shallow
    for g in range(n_groups):
        seq = feat.reshape(B, C, H * W).transpose(1, 2)
        for j in range(n_blocks):
            seq = _block(sd, f'groups.{g}.blocks.{j}', seq, H, W, j % 2 == 0, heads, ws)
        feat = _conv(sd, f'groups.{g}.conv', seq.transpose(1, 2).reshape(B, C, H, W)) + feat
    y = _upsampler(sd, _conv(sd, 'conv_after', feat) + shallow, mode, scale, dim, out, mid)
    return y[:, :, : h * report, : w * report]
