"""A functional restatement of FlexNet's linear pipeline in plain torch, written from the math (not from the reference's module code): the
reflect pad to a multiple of 8, short_cut and in_to_feat, the LBlocks of TransformerBlocks with their ConvBlock, the three heads and the
crop.  It runs in the dtype of ``x`` (f32 or f64).  RMSNorm's eps is 2^-23 whatever the dtype: that is what the reference's
``nn.RMSNorm(eps=None)`` uses in the f32 it runs in (a ``.double()`` copy of the reference silently uses 2^-52).  OmniShift is always
rebuilt from its training parameters: the stored ``conv5x5_reparam`` is never read.  No einops."""

import math

import torch
import torch.nn.functional as F

from rha_oracle import dysample  # the shared DySample head (utilities/dysample.py, 4 groups), already restated there

EPS = 2.0**-23
WS = 8


def hyper(sd):
    dim, in_ch = (int(v) for v in sd['in_to_feat.weight'].shape[:2])
    n_l = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('pipeline.att.'))
    blocks = [1 + max(int(k.split('.')[4]) for k in sd if k.startswith(f'pipeline.att.{i}.t_blocks.')) for i in range(n_l)]
    hidden = int(sd['pipeline.att.0.t_blocks.0.ffn.key.weight'].shape[0])
    out_ch = in_ch
    if 'to_img.1.0.weight' in sd:
        head, scale = 'n+c', int(sd['scale_factor'])
        last = max(int(k.split('.')[2]) for k in sd if k.startswith('to_img.1.'))
        out_ch = int(sd[f'to_img.1.{last}.weight'].shape[0])
    elif 'to_img.init_pos' in sd:
        head, scale, out_ch = 'dys', math.isqrt(int(sd['to_img.offset.weight'].shape[0]) // 8), int(sd['to_img.end_conv.weight'].shape[0])
    else:
        head, scale = 'ps', math.isqrt(int(sd['to_img.0.weight'].shape[0]) // out_ch)
    return dict(dim=dim, in_ch=in_ch, out_ch=out_ch, blocks=blocks, hidden=hidden, hidden_rate=hidden // dim, head=head, scale=scale,
                channel_norm='pipeline.att.0.t_blocks.0.ffn.key_norm.weight' in sd, window=int(sd['window_size']))  # fmt: skip


def rmsnorm(x, w, dim=1):
    """x * rsqrt(mean(x^2) + eps) * w over ``dim``."""
    shape = [1] * x.dim()
    shape[dim] = -1
    return x * torch.rsqrt((x * x).mean(dim, keepdim=True) + EPS) * w.to(x.dtype).reshape(shape)


def omnishift(sd, key, x):
    """alpha0 x + alpha1 dw1(x) + alpha2 dw3(x) + alpha3 dw5(x), as one bias-free 5x5 depthwise kernel, zero padding 2."""
    t, c = x.dtype, x.shape[1]
    a = sd[f'{key}.alpha'].to(t)
    ident = torch.zeros((c, 1, 5, 5), dtype=t)
    ident[:, :, 2, 2] = 1
    w = a[0] * ident + a[1] * F.pad(sd[f'{key}.conv1x1.weight'].to(t), (2, 2, 2, 2)) + a[2] * F.pad(sd[f'{key}.conv3x3.weight'].to(t), (1, 1, 1, 1))
    w = w + a[3] * sd[f'{key}.conv5x5.weight'].to(t)
    return F.conv2d(x, w, None, padding=2, groups=c)


def window_attention(sd, key, x):
    """softmax(q k^T / sqrt(C)) v + lepe(v) on every 8 x 8 window of x [B, C, H, W], one head; lepe convolves each window as its own image."""
    t = x.dtype
    B, C, H, W = x.shape
    win = x.reshape(B, C, H // WS, WS, W // WS, WS).permute(0, 2, 4, 3, 5, 1).reshape(-1, WS * WS, C)
    qkv = win @ sd[f'{key}.qkv.weight'].to(t).T + sd[f'{key}.qkv.bias'].to(t)
    q, k, v = qkv[..., :C], qkv[..., C : 2 * C], qkv[..., 2 * C :]
    vi = v.transpose(1, 2).reshape(-1, C, WS, WS)
    lepe = F.conv2d(vi, sd[f'{key}.get_v.weight'].to(t), sd[f'{key}.get_v.bias'].to(t), padding=1, groups=C).reshape(-1, C, WS * WS).transpose(1, 2)
    att = torch.softmax((q @ k.transpose(1, 2)) * C**-0.5, dim=-1)
    o = (att @ v + lepe) @ sd[f'{key}.proj.weight'].to(t).T + sd[f'{key}.proj.bias'].to(t)
    return o.reshape(B, H // WS, W // WS, WS, WS, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


def channel_mix(sd, key, x):
    t = x.dtype
    s = omnishift(sd, f'{key}.omni_shift', x).permute(0, 2, 3, 1)  # [B, H, W, C]
    k = torch.relu(s @ sd[f'{key}.key.weight'].to(t).T) ** 2
    if f'{key}.key_norm.weight' in sd:
        k = rmsnorm(k, sd[f'{key}.key_norm.weight'], dim=-1)
    o = torch.sigmoid(s @ sd[f'{key}.receptance.weight'].to(t).T) * (k @ sd[f'{key}.value.weight'].to(t).T)
    return o.permute(0, 3, 1, 2)


def transformer_block(sd, key, x):
    t = x.dtype
    g1, g2 = (sd[f'{key}.gamma{i}'].to(t).reshape(1, -1, 1, 1) for i in (1, 2))
    x = x + g1 * window_attention(sd, f'{key}.att', omnishift(sd, f'{key}.att.omni_shift', rmsnorm(x, sd[f'{key}.rn1.weight'])))
    return x + g2 * channel_mix(sd, f'{key}.ffn', rmsnorm(x, sd[f'{key}.rn2.weight']))


def conv(sd, key, x, padding):
    return F.conv2d(x, sd[f'{key}.weight'].to(x.dtype), sd[f'{key}.bias'].to(x.dtype), padding=padding)


def convblock(sd, key, x):
    return F.mish(conv(sd, f'{key}.block.2', F.mish(conv(sd, f'{key}.block.0', x, 1)), 1)) + conv(sd, f'{key}.conv11', x, 0)


def flexnet_forward(sd, x):
    hp = hyper(sd)
    if hp['window'] != WS:
        raise ValueError('the reference runs window_size 8 only')
    _, _, h, w = x.shape
    x = F.pad(x, (0, (WS - w % WS) % WS, 0, (WS - h % WS) % WS), 'reflect')
    short = convblock(sd, 'short_cut', x)
    f = conv(sd, 'in_to_feat', x, 1)
    for li, nb in enumerate(hp['blocks']):
        inp = f
        for bi in range(nb):
            f = transformer_block(sd, f'pipeline.att.{li}.t_blocks.{bi}', f)
        f = convblock(sd, f'pipeline.att.{li}.conv', torch.cat([inp, f], 1))
    f = torch.cat([f, short], 1)
    s = hp['scale']
    if hp['head'] == 'ps':
        y = F.pixel_shuffle(conv(sd, 'to_img.0', f, 1), s)
    elif hp['head'] == 'dys':
        y = dysample(sd, 'to_img', f, s)
    else:
        y = conv(sd, 'to_img.0', f, 1)
        idx = sorted(int(k.split('.')[2]) for k in sd if k.startswith('to_img.1.') and k.endswith('.weight'))
        for j, i in enumerate(idx[:-1]):
            y = conv(sd, f'to_img.1.{i}', y, 1)
            if j < len(idx) - 2:  # every convolution but the last two is followed by the nearest upsampling
                y = F.interpolate(y, scale_factor=3 if s == 3 else 2, mode='nearest')
            y = F.leaky_relu(y, 0.2)
        y = conv(sd, f'to_img.1.{idx[-1]}', y, 1)
    return y[:, :, : h * s, : w * s]
