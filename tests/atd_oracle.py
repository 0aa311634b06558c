"""Plain-torch functional oracle of ATD (reference resselt/archs/atd/arch.py in eval mode), written from the state dict.

It differs from the reference in one defined way: tokens are sorted by category with a STABLE sort (ascending token index inside a
category); the reference calls ``torch.sort(stable=False)``, whose order is not a function of its input.  ``force`` replaces the oracle's
own argmax + sort by given permutations (one [b, n] integer tensor per layer, in forward order), which is how parity with a recorded run of
the real reference is checked.  ``record`` (a dict) receives per layer the ids, the permutation used and the smallest relative top-two
margin of the similarity map.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

RGB_MEAN = (0.4488, 0.4371, 0.4040)
TAU = 1e-4  # near-tie threshold of a sim row: (largest - second largest) / largest


def hyper_of(model) -> dict:
    """The hyper-parameters the oracle needs, from an engine (or reference) ATD module."""
    return dict(window_size=model.window_size, category_size=getattr(model, 'category_size', None), upscale=model.upscale, upsampler=model.upsampler,
                img_range=model.img_range, norm=bool(model.is_norm))  # fmt: skip


def top2_margin(sim: torch.Tensor) -> torch.Tensor:
    """Relative difference of the two largest values of every row of sim [..., m]."""
    t = sim.topk(2, dim=-1).values
    return (t[..., 0] - t[..., 1]) / t[..., 0]


def _seq_len(sd, prefix):
    k = 0
    while any(key.startswith(f'{prefix}.{k}.') for key in sd):
        k += 1
    return k


def _lin(sd, name, x):
    return F.linear(x, sd[f'{name}.weight'], sd.get(f'{name}.bias'))


def _resi(sd, name, x):
    if f'{name}.weight' in sd:
        return F.conv2d(x, sd[f'{name}.weight'], sd[f'{name}.bias'], padding=1)
    x = F.leaky_relu(F.conv2d(x, sd[f'{name}.0.weight'], sd[f'{name}.0.bias'], padding=1), 0.2)
    x = F.leaky_relu(F.conv2d(x, sd[f'{name}.2.weight'], sd[f'{name}.2.bias']), 0.2)
    return F.conv2d(x, sd[f'{name}.4.weight'], sd[f'{name}.4.bias'], padding=1)


def _shift_mask(h, w, ws, like):
    img = torch.zeros(h, w, dtype=like.dtype, device=like.device)
    cnt = 0
    for a in (slice(0, -ws), slice(-ws, -(ws // 2)), slice(-(ws // 2), None)):
        for b in (slice(0, -ws), slice(-ws, -(ws // 2)), slice(-(ws // 2), None)):
            img[a, b] = cnt
            cnt += 1
    mw = img.view(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    d = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def _windows(t, ws):
    b, h, w, c = t.shape
    return t.view(b, h // ws, ws, w // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, c)


def _layer(sd, p, x, td, hw, heads, ws, shift, cat_size, rpi, last, force, record):
    h, w = hw
    b, n, c = x.shape
    hd = c // heads
    shortcut = x
    xn = F.layer_norm(x, (c,), sd[f'{p}.norm1.weight'], sd[f'{p}.norm1.bias'])
    qkv = _lin(sd, f'{p}.wqkv', xn)
    # ATD_CA
    m = td.shape[1]
    q = _lin(sd, f'{p}.attn_atd.wq', xn)
    k = _lin(sd, f'{p}.attn_atd.wk', td)
    v = _lin(sd, f'{p}.attn_atd.wv', td)
    attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    attn = attn * (1 + torch.clamp(sd[f'{p}.attn_atd.scale'], 0, 1) * math.log(m))
    sim = attn.softmax(-1)
    x_atd = sim @ v
    # AC_MSA
    gs = min(n, cat_size)
    ng = (n + gs - 1) // gs
    ids = sim.argmax(-1)
    if force is not None:
        perm = force.to(torch.long).reshape(b, n)
    else:
        perm = torch.sort(ids, dim=-1, stable=True).indices
    if record is not None:
        record.setdefault('ids', []).append(ids.clone())
        record.setdefault('perm', []).append(perm.clone())
        record.setdefault('margin', []).append(top2_margin(sim))
        record.setdefault('sim', []).append(sim)
    inv = torch.empty_like(perm)
    inv.scatter_(1, perm, torch.arange(n, device=perm.device).expand(b, n))
    sh = torch.gather(qkv, 1, perm[..., None].expand(-1, -1, 3 * c))
    pad_n = ng * gs - n
    padded = torch.cat((sh, torch.flip(sh[:, n - pad_n : n], dims=[1])), dim=1)
    y = padded.reshape(b, ng, gs, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)
    a = (y[0] @ y[1].transpose(-2, -1)) * torch.clamp(sd[f'{p}.attn_aca.logit_scale'], max=math.log(100.0)).exp()
    y = (a.softmax(-1) @ y[2]).permute(0, 1, 3, 2, 4).reshape(b, n + pad_n, c)[:, :n]
    x_aca = _lin(sd, f'{p}.attn_aca.proj', torch.gather(y, 1, inv[..., None].expand(-1, -1, c)))
    # SW-MSA
    t = qkv.reshape(b, h, w, 3 * c)
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    xw = _windows(t, ws)
    nw = xw.shape[0]
    y = xw.reshape(nw, ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = (y[0] * hd**-0.5) @ y[1].transpose(-2, -1)
    bias = sd[f'{p}.attn_win.relative_position_bias_table'][rpi.reshape(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1)
    a = a + bias.unsqueeze(0)
    if shift:
        mask = _shift_mask(h, w, ws, a)
        a = (a.view(nw // mask.shape[0], mask.shape[0], heads, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)).view(nw, heads, ws * ws, ws * ws)
    y = (a.softmax(-1) @ y[2]).transpose(1, 2).reshape(nw, ws * ws, c)
    y = _lin(sd, f'{p}.attn_win.proj', y)
    y = y.view(b, h // ws, w // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    x = shortcut + y.reshape(b, n, c) + x_atd + x_aca
    # ConvFFN
    f = F.gelu(_lin(sd, f'{p}.convffn.fc1', F.layer_norm(x, (c,), sd[f'{p}.norm2.weight'], sd[f'{p}.norm2.bias'])))
    hid = f.shape[-1]
    dw = sd[f'{p}.convffn.dwconv.depthwise_conv.0.weight']
    g = F.conv2d(f.transpose(1, 2).reshape(b, hid, h, w), dw, sd[f'{p}.convffn.dwconv.depthwise_conv.0.bias'], padding=(dw.shape[2] - 1) // 2, groups=hid)
    f = f + F.gelu(g).flatten(2).transpose(1, 2)
    x = x + _lin(sd, f'{p}.convffn.fc2', f)
    if not last:
        z = F.instance_norm(sim.transpose(-1, -2), weight=sd[f'{p}.norm3.weight'], bias=sd[f'{p}.norm3.bias'], eps=1e-5)
        s = torch.sigmoid(sd[f'{p}.sigma'])
        td = s * td + (1 - s) * torch.einsum('btn,bnc->btc', z.softmax(-1), x)
    return x, td


def atd_forward(sd: dict, x: torch.Tensor, hyper: dict, force: list | None = None, record: dict | None = None) -> torch.Tensor:
    sd = {k: v.detach().to(x.dtype) if v.is_floating_point() else v for k, v in sd.items()}
    ws, s, up = hyper['window_size'], hyper['upscale'], hyper['upsampler']
    rng = hyper.get('img_range', 1.0)
    c_in = sd['conv_first.weight'].shape[1]
    embed = sd['conv_first.weight'].shape[0]
    cat_size = hyper.get('category_size') or (128 if up == 'pixelshuffledirect' and embed == 48 else 256)
    h0, w0 = x.shape[-2:]
    h, w = (h0 + ws - 1) // ws * ws, (w0 + ws - 1) // ws * ws
    x = torch.cat([x, torch.flip(x, [2])], 2)[:, :, :h]
    x = torch.cat([x, torch.flip(x, [3])], 3)[:, :, :, :w]
    mean = torch.tensor(RGB_MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) if c_in == 3 else torch.zeros(1, 1, 1, 1, dtype=x.dtype, device=x.device)
    if hyper.get('norm', True):
        x = (x - mean) * rng
    rpi = sd['relative_position_index_SA']
    first = F.conv2d(x, sd['conv_first.weight'], sd['conv_first.bias'], padding=1)
    t = first.flatten(2).transpose(1, 2)
    if 'patch_embed.norm.weight' in sd:
        t = F.layer_norm(t, (embed,), sd['patch_embed.norm.weight'], sd['patch_embed.norm.bias'])
    li = 0
    for i in range(_seq_len(sd, 'layers')):
        g = f'layers.{i}.residual_group'
        depth = _seq_len(sd, f'{g}.layers')
        heads = sd[f'{g}.layers.0.attn_win.relative_position_bias_table'].shape[1]
        td = sd[f'{g}.td'].repeat([t.shape[0], 1, 1])
        u = t
        for j in range(depth):
            u, td = _layer(sd, f'{g}.layers.{j}', u, td, (h, w), heads, ws, 0 if j % 2 == 0 else ws // 2, cat_size, rpi, j == depth - 1,
                           None if force is None else force[li], record)  # fmt: skip
            li += 1
        t = _resi(sd, f'layers.{i}.conv', u.transpose(1, 2).reshape(-1, embed, h, w)).flatten(2).transpose(1, 2) + t
    t = F.layer_norm(t, (embed,), sd['norm.weight'], sd['norm.bias']).transpose(1, 2).reshape(-1, embed, h, w)
    if up == '':
        y = x + F.conv2d(_resi(sd, 'conv_after_body', t) + first, sd['conv_last.weight'], sd['conv_last.bias'], padding=1)
    else:
        y = _resi(sd, 'conv_after_body', t) + first
        if up == 'pixelshuffle':
            y = F.leaky_relu(F.conv2d(y, sd['conv_before_upsample.0.weight'], sd['conv_before_upsample.0.bias'], padding=1), 0.01)
            k = 0
            while f'upsample.{k}.weight' in sd:
                wgt = sd[f'upsample.{k}.weight']
                y = F.pixel_shuffle(F.conv2d(y, wgt, sd[f'upsample.{k}.bias'], padding=1), math.isqrt(wgt.shape[0] // wgt.shape[1]))
                k += 2
            y = F.conv2d(y, sd['conv_last.weight'], sd['conv_last.bias'], padding=1)
        elif up == 'pixelshuffledirect':
            y = F.pixel_shuffle(F.conv2d(y, sd['upsample.0.weight'], sd['upsample.0.bias'], padding=1), s)
        else:  # nearest+conv
            y = F.leaky_relu(F.conv2d(y, sd['conv_before_upsample.0.weight'], sd['conv_before_upsample.0.bias'], padding=1), 0.01)
            for name in ('conv_up1', 'conv_up2'):
                y = F.leaky_relu(F.conv2d(F.interpolate(y, scale_factor=2, mode='nearest'), sd[f'{name}.weight'], sd[f'{name}.bias'], padding=1), 0.2)
            y = F.conv2d(F.leaky_relu(F.conv2d(y, sd['conv_hr.weight'], sd['conv_hr.bias'], padding=1), 0.2), sd['conv_last.weight'], sd['conv_last.bias'], padding=1)
    if hyper.get('norm', True):
        y = y / rng + mean
    return y[..., : h0 * s, : w0 * s]
