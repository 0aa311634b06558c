"""Plain-torch restatement of RGT in eval mode (reference archs/rgt/arch.py:630-838), written from the module's equations rather than
its code: the L_SA windows are built by explicit padding, rolling and unfolding, RG-SA's recursion, CPE and cross-attention are spelled
out per head.  Pinned to every tests/golden/rgt_*.npz fixture by tests/test_rgt_loader.py; the GPU tests use it where no fixture exists.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

RGB_MEAN = (0.4488, 0.4371, 0.4040)


def _ln(x, sd, name):  # x [..., C]
    return F.layer_norm(x, (x.shape[-1],), sd[f'{name}.weight'], sd[f'{name}.bias'], 1e-5)


def _lin(x, sd, name):
    return F.linear(x, sd[f'{name}.weight'], sd.get(f'{name}.bias'))


def _dw(x, sd, name, stride=1, pad=1):  # x [B, C, H, W]
    return F.conv2d(x, sd[f'{name}.weight'], sd[f'{name}.bias'], stride=stride, padding=pad, groups=x.shape[1])


def _pos_bias(sd, a, hs, ws):
    pos = _lin(sd[f'{a}.rpe_biases'], sd, f'{a}.pos.pos_proj')
    for k in ('pos1', 'pos2', 'pos3'):
        pos = _lin(F.relu(_ln(pos, sd, f'{a}.pos.{k}.0')), sd, f'{a}.pos.{k}.2')
    ys, xs = torch.meshgrid(torch.arange(hs), torch.arange(ws), indexing='ij')
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    idx = (ys[:, None] - ys[None, :] + hs - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)
    return pos[idx].permute(2, 0, 1)  # [heads, N, N]


def _region_ids(Hp, Wp, hs, ws, sh, sw):
    r = torch.zeros(Hp, Wp, dtype=torch.long)
    yb = torch.where(torch.arange(Hp) < Hp - hs, 0, torch.where(torch.arange(Hp) < Hp - sh, 1, 2))
    xb = torch.where(torch.arange(Wp) < Wp - ws, 0, torch.where(torch.arange(Wp) < Wp - sw, 1, 2))
    return r + yb[:, None] * 3 + xb[None, :]


def _window_attention(q, k, v, bias, hs, ws, shift, heads, scale):
    """q, k, v [B, Hp, Wp, c] (c = heads * hd), windows of hs x ws after rolling by -shift; returns [B, Hp, Wp, c] rolled back."""
    B, Hp, Wp, c = q.shape
    sh, sw = shift
    if sh or sw:
        q, k, v = (torch.roll(t, (-sh, -sw), (1, 2)) for t in (q, k, v))

    def win(t):
        return t.reshape(B, Hp // hs, hs, Wp // ws, ws, heads, c // heads).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, Hp // hs, Wp // ws, heads, hs * ws, c // heads)

    qw, kw, vw = win(q), win(k), win(v)
    s = (qw * scale) @ kw.transpose(-1, -2) + bias
    if sh or sw:
        reg = _region_ids(Hp, Wp, hs, ws, sh, sw).reshape(Hp // hs, hs, Wp // ws, ws).permute(0, 2, 1, 3).reshape(Hp // hs, Wp // ws, 1, hs * ws)
        s = s + torch.zeros((), dtype=s.dtype, device=s.device).masked_fill(reg[..., :, None] != reg[..., None, :], -100.0)
    o = torch.softmax(s, -1) @ vw
    o = o.reshape(B, Hp // hs, Wp // ws, heads, hs, ws, c // heads).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, c)
    if sh or sw:
        o = torch.roll(o, (sh, sw), (1, 2))
    return o


def _shifted(rs: int, idx: int) -> bool:
    return (rs % 2 == 0 and idx > 0 and (idx - 2) % 4 == 0) or (rs % 2 != 0 and idx % 4 == 0)


def l_sa(x, sd, a, H, W, heads, split, shifted):
    B, N, C = x.shape
    q, k, v = _lin(x, sd, f'{a}.qkv').reshape(B, H, W, 3, C).unbind(3)
    m = max(split)
    Hp, Wp = H + (m - H % m) % m, W + (m - W % m) % m
    pad = lambda t: F.pad(t, (0, 0, 0, Wp - W, 0, Hp - H))  # noqa: E731  (zeros AFTER qkv)
    qp, kp, vp = pad(q), pad(k), pad(v)
    outs = []
    hd = C // heads
    for idx, (hs, ws) in enumerate(((split[0], split[1]), (split[1], split[0]))):
        sl = slice(idx * C // 2, (idx + 1) * C // 2)
        shift = (hs // 2, ws // 2) if shifted else (0, 0)
        bias = _pos_bias(sd, f'{a}.attns.{idx}', hs, ws)
        outs.append(_window_attention(qp[..., sl], kp[..., sl], vp[..., sl], bias, hs, ws, shift, heads // 2, hd**-0.5)[:, :H, :W])
    att = torch.cat(outs, -1).reshape(B, N, C)
    lcm = _dw(v.permute(0, 3, 1, 2), sd, f'{a}.get_v').permute(0, 2, 3, 1).reshape(B, N, C)
    return _lin(att + lcm, sd, f'{a}.proj')


def rg_sa(x, sd, a, H, W, heads, c_ratio):
    B, N, C = x.shape
    cr = sd[f'{a}.q.weight'].shape[0]
    t = max(int(math.log(H // 16, 4)), int(math.log(W // 16, 4)))
    t = max(t, 2)
    y = x.transpose(1, 2).reshape(B, C, H, W)
    for _ in range(t):
        y = _dw(y, sd, f'{a}.reduction1', stride=4, pad=0)
    hs, ws = y.shape[-2:]
    y = F.conv2d(_dw(y, sd, f'{a}.dwconv'), sd[f'{a}.conv.weight'], sd[f'{a}.conv.bias'])
    y = F.gelu(_ln(y.flatten(2).transpose(1, 2), sd, f'{a}.norm_act.0'))  # [B, N', cr]
    q = _lin(x, sd, f'{a}.q').reshape(B, N, heads, cr // heads).transpose(1, 2)
    k = _lin(y, sd, f'{a}.k').reshape(B, -1, heads, cr // heads).transpose(1, 2)
    v = _lin(y, sd, f'{a}.v')  # [B, N', C]
    vm = v.transpose(1, 2).reshape(B, C, hs, ws)
    v = (vm + _dw(vm, sd, f'{a}.cpe')).flatten(2).reshape(B, heads, C // heads, -1).transpose(-1, -2)
    scale = (C // heads * c_ratio) ** -0.5
    o = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v
    return _lin(o.transpose(1, 2).reshape(B, N, C), sd, f'{a}.proj')


def _mlp(x, sd, m, H, W):
    B, N, _ = x.shape
    h = F.gelu(_lin(x, sd, f'{m}.fc1'))
    x1, x2 = h.chunk(2, -1)
    x2 = _dw(_ln(x2, sd, f'{m}.sg.norm').transpose(1, 2).reshape(B, -1, H, W), sd, f'{m}.sg.conv').flatten(2).transpose(1, 2)
    return _lin(x1 * x2, sd, f'{m}.fc2')


def _resi(x, sd, name):
    if f'{name}.weight' in sd:
        return F.conv2d(x, sd[f'{name}.weight'], sd[f'{name}.bias'], padding=1)
    y = F.leaky_relu(F.conv2d(x, sd[f'{name}.0.weight'], sd[f'{name}.0.bias'], padding=1), 0.2)
    y = F.leaky_relu(F.conv2d(y, sd[f'{name}.2.weight'], sd[f'{name}.2.bias']), 0.2)
    return F.conv2d(y, sd[f'{name}.4.weight'], sd[f'{name}.4.bias'], padding=1)


def rgt_forward(sd, x, split_size, num_heads, c_ratio):
    sd = {k: v.to(x.dtype) for k, v in sd.items()}  # the arithmetic runs in the input's dtype
    B, cin, H, W = x.shape
    mean = torch.tensor(RGB_MEAN if cin == 3 else [0.0] * cin, dtype=x.dtype, device=x.device).view(1, cin, 1, 1)
    x = x - mean
    first = F.conv2d(x, sd['conv_first.weight'], sd['conv_first.bias'], padding=1)
    C = first.shape[1]
    t = _ln(first.flatten(2).transpose(1, 2), sd, 'before_RG.1')
    i = 0
    while f'layers.{i}.conv.weight' in sd or f'layers.{i}.conv.0.weight' in sd:
        rg_in = t
        j = 0
        while f'layers.{i}.blocks.{j}.norm1.weight' in sd:
            b = f'layers.{i}.blocks.{j}'
            res = t
            n1 = _ln(t, sd, f'{b}.norm1')
            if j % 2 == 0:
                t = t + l_sa(n1, sd, f'{b}.attn', H, W, num_heads[i], split_size, _shifted(i, j))
            else:
                t = t + rg_sa(n1, sd, f'{b}.attn', H, W, num_heads[i], c_ratio)
            t = t + _mlp(_ln(t, sd, f'{b}.norm2'), sd, f'{b}.mlp', H, W)
            t = t + res * sd[f'{b}.gamma']
            j += 1
        t = rg_in + _resi(t.transpose(1, 2).reshape(B, C, H, W), sd, f'layers.{i}.conv').flatten(2).transpose(1, 2)
        i += 1
    y = _ln(t, sd, 'norm').transpose(1, 2).reshape(B, C, H, W)
    y = _resi(y, sd, 'conv_after_body') + first
    y = F.leaky_relu(F.conv2d(y, sd['conv_before_upsample.0.weight'], sd['conv_before_upsample.0.bias'], padding=1), 0.01)
    u = 0
    while f'upsample.{u}.weight' in sd:
        w = sd[f'upsample.{u}.weight']
        y = F.pixel_shuffle(F.conv2d(y, w, sd[f'upsample.{u}.bias'], padding=1), math.isqrt(w.shape[0] // w.shape[1]))
        u += 2
    y = F.conv2d(y, sd['conv_last.weight'], sd['conv_last.bias'], padding=1)
    return y + mean
