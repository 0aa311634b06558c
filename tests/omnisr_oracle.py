"""Plain-torch OmniSR forward (reference ``resselt/archs/omni/arch.py``, eval mode) from a state dict: the CPU oracle of the OmniSR tests.

It does not import the reference.  Hyper-parameters are read from the state dict the way the loader reads them (omni/__init__.py).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

HEADS = 4


def _seq_len(sd, prefix):
    return 1 + max(int(k[len(prefix) + 1 :].split('.')[0]) for k in sd if k.startswith(prefix + '.'))


def _conv(sd, name, x, stride=1, pad=None, groups=1):
    w = sd[f'{name}.weight']
    return F.conv2d(x, w, sd.get(f'{name}.bias'), stride=stride, padding=w.shape[-1] // 2 if pad is None else pad, groups=groups)


def _ln_channels(x, w, b, eps):
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def _mbconv(sd, p, x):
    h = F.gelu(_conv(sd, f'{p}.0', x))
    h = F.gelu(_conv(sd, f'{p}.2', h, groups=h.shape[1]))
    g = torch.sigmoid(F.linear(F.silu(F.linear(h.mean((2, 3)), sd[f'{p}.4.gate.1.weight'])), sd[f'{p}.4.gate.3.weight']))
    return x + _conv(sd, f'{p}.5', h * g[:, :, None, None])


def _windows(x, ws, grid):
    """[b, d, H, W] -> [b * nwin, ws * ws, d]: block 'b d (x w1) (y w2)', grid 'b d (w1 x) (w2 y)'."""
    b, d, H, W = x.shape
    if grid:
        t = x.view(b, d, ws, H // ws, ws, W // ws).permute(0, 3, 5, 2, 4, 1)
    else:
        t = x.view(b, d, H // ws, ws, W // ws, ws).permute(0, 2, 4, 3, 5, 1)
    return t.reshape(-1, ws * ws, d)


def _unwindows(t, b, H, W, ws, grid):
    d = t.shape[-1]
    t = t.view(b, H // ws, W // ws, ws, ws, d)
    if grid:
        return t.permute(0, 5, 3, 1, 4, 2).reshape(b, d, H, W)
    return t.permute(0, 5, 1, 3, 2, 4).reshape(b, d, H, W)


def _attention(sd, p, x, ws, grid):
    b, c, H, W = x.shape
    n = _ln_channels(x, sd[f'{p}.norm.weight'], sd[f'{p}.norm.bias'], 1e-5)
    t = _windows(n, ws, grid)
    q, k, v = F.linear(t, sd[f'{p}.fn.to_qkv.weight']).chunk(3, dim=-1)
    q, k, v = (u.view(u.shape[0], -1, HEADS, c // HEADS).transpose(1, 2) for u in (q, k, v))
    sim = (q * (c // HEADS) ** -0.5) @ k.transpose(-1, -2)
    key = f'{p}.fn.rel_pos_bias.weight'
    if key in sd:
        pos = torch.stack(torch.meshgrid(torch.arange(ws, device=x.device), torch.arange(ws, device=x.device), indexing='ij')).reshape(2, -1)
        rel = pos[:, :, None] - pos[:, None, :] + ws - 1
        sim = sim + sd[key][rel[0] * (2 * ws - 1) + rel[1]].permute(2, 0, 1)
    o = (sim.softmax(-1) @ v).transpose(1, 2).reshape(t.shape[0], -1, c)
    return x + _unwindows(F.linear(o, sd[f'{p}.fn.to_out.0.weight']), b, H, W, ws, grid)


def _channel_attention(sd, p, x, ws, grid):
    b, c, H, W = x.shape
    n = _ln_channels(x, sd[f'{p}.norm.weight'], sd[f'{p}.norm.bias'], 1e-6)
    qkv = F.conv2d(F.conv2d(n, sd[f'{p}.fn.qkv.weight']), sd[f'{p}.fn.qkv_dwconv.weight'], padding=1, groups=3 * c)
    d, gh, gw = c // HEADS, H // ws, W // ws

    def split(t):  # -> [b, sets, heads, d, tokens]
        t = t.view(b, HEADS, d, gh, ws, gw, ws)
        if grid:  # 'b (head d) (h ph) (w pw) -> b (ph pw) head d (h w)'
            return t.permute(0, 4, 6, 1, 2, 3, 5).reshape(b, ws * ws, HEADS, d, gh * gw)
        return t.permute(0, 3, 5, 1, 2, 4, 6).reshape(b, gh * gw, HEADS, d, ws * ws)

    q, k, v = (split(t) for t in qkv.chunk(3, dim=1))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = (q @ k.transpose(-1, -2)) * sd[f'{p}.fn.temperature'].view(1, 1, HEADS, 1, 1)
    o = attn.softmax(-1) @ v
    if grid:
        o = o.view(b, ws, ws, HEADS, d, gh, gw).permute(0, 3, 4, 5, 1, 6, 2)
    else:
        o = o.view(b, gh, gw, HEADS, d, ws, ws).permute(0, 3, 4, 1, 5, 2, 6)
    return x + F.conv2d(o.reshape(b, c, H, W), sd[f'{p}.fn.project_out.weight'])


def _ffn(sd, p, x):
    c = x.shape[1]
    n = _ln_channels(x, sd[f'{p}.norm.weight'], sd[f'{p}.norm.bias'], 1e-6)
    x1, x2 = F.conv2d(F.conv2d(n, sd[f'{p}.fn.project_in.weight']), sd[f'{p}.fn.dwconv.weight'], padding=1, groups=2 * c).chunk(2, dim=1)
    return x + F.conv2d(F.gelu(x1) * x2, sd[f'{p}.fn.project_out.weight'])


def _esa(sd, p, x):
    c1_ = _conv(sd, f'{p}.conv1', x)
    c1 = _conv(sd, f'{p}.conv2', c1_, stride=2, pad=0)
    c3 = _conv(sd, f'{p}.conv3', F.max_pool2d(c1, kernel_size=7, stride=3))
    c3 = F.interpolate(c3, x.shape[2:], mode='bilinear', align_corners=False)
    return x * torch.sigmoid(_conv(sd, f'{p}.conv4', c3 + _conv(sd, f'{p}.conv_f', c1_)))


def omnisr_forward(sd, x):
    sd = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith(('total_ops', 'total_params'))}
    c_in = sd['input.weight'].shape[1]
    scale = math.isqrt(sd['up.0.weight'].shape[0] // c_in)
    key = 'residual_layer.0.residual_layer.0.layer.2.fn.rel_pos_bias.weight'
    ws = int((math.sqrt(sd[key].shape[0]) + 1) / 2) if key in sd else 8
    res_num = _seq_len(sd, 'residual_layer')
    block_num = _seq_len(sd, 'residual_layer.0.residual_layer') - 1
    h, w = x.shape[2:]
    x = F.pad(x, (0, (ws - w % ws) % ws, 0, (ws - h % ws) % ws))
    residual = _conv(sd, 'input', x)
    out = residual
    for g in range(res_num):
        t = out
        for j in range(block_num):
            p = f'residual_layer.{g}.residual_layer.{j}.layer'
            t = _mbconv(sd, f'{p}.0.fn', t)
            t = _attention(sd, f'{p}.2', t, ws, False)
            t = _ffn(sd, f'{p}.4', t)
            t = _channel_attention(sd, f'{p}.5', t, ws, False)
            t = _ffn(sd, f'{p}.6', t)
            t = _attention(sd, f'{p}.8', t, ws, True)
            t = _ffn(sd, f'{p}.10', t)
            t = _channel_attention(sd, f'{p}.11', t, ws, True)
            t = _ffn(sd, f'{p}.12', t)
        t = _conv(sd, f'residual_layer.{g}.residual_layer.{block_num}', t) + out
        out = _esa(sd, f'residual_layer.{g}.esa', t)
    out = _conv(sd, 'output', out) + residual
    y = F.pixel_shuffle(_conv(sd, 'up.0', out), scale)
    return y[:, :, : h * scale, : w * scale]
