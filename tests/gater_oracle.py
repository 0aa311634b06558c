"""Plain-torch GateR forward from a state dict (eval mode), in the dtype of the input: the CPU oracle of the GateR tests.

Written from the semantics (U-shaped restoration network of gated blocks ``x + fc2(mish(g) * cat(i, mix(c)))`` behind torch's RMSNorm, where
``mix`` is a 7x7 depthwise convolution or, in the latent stage of a ``latent_att`` checkpoint, a focused linear attention over all tokens),
not from the reference's text.  Usable in f32 and f64: every weight is cast to the input's dtype.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F  # noqa: N812

HEADS = 8


def seq_len(sd, prefix: str) -> int:
    return len({k[len(prefix) + 1 :].split('.')[0] for k in sd if k.startswith(prefix + '.')})


def focus(t, scale, factor):
    """Whole tokens [B, N, C]: relu + 1e-6, / softplus(scale), per-channel power, renormalised to the norm before the power."""
    t = (F.relu(t) + 1e-6) / F.softplus(scale)
    n0 = t.norm(dim=-1, keepdim=True)
    t = t**factor
    return t / t.norm(dim=-1, keepdim=True) * n0


def focused_linear_attention(w, c, hw):
    """c [B, N, C] -> [B, N, C] (before ``proj``): (q KV) z per head with KV = k^T v / n, z = 1 / (q . mean(k) + 1e-6), plus the 5x5
    depthwise convolution of v whose C / 8 filters every head shares."""
    B, N, C = c.shape
    d = C // HEADS
    q = focus(F.linear(c, w('q.weight'), w('q.bias')), w('scale'), w('focusing_factor'))
    kv = F.linear(c, w('kv.weight'), w('kv.bias'))
    k, v = focus(kv[..., :C], w('scale'), w('focusing_factor')), kv[..., C:]
    qh, kh, vh = (t.reshape(B, N, HEADS, d).transpose(1, 2) for t in (q, k, v))  # [B, heads, N, d]
    z = 1.0 / ((qh * kh.mean(dim=2, keepdim=True)).sum(-1, keepdim=True) + 1e-6)
    kvm = kh.transpose(-2, -1) @ vh / N
    out = (qh @ kvm * z).transpose(1, 2).reshape(B, N, C)
    vmap = v.transpose(1, 2).reshape(B, C, *hw)
    dw = F.conv2d(vmap, w('dwc.weight').repeat(HEADS, 1, 1, 1), w('dwc.bias').repeat(HEADS), padding=2, groups=C)
    return out + dw.flatten(2).transpose(1, 2)


def gated_block(sd, p, x, hw, dt):
    """x [B, N, C] tokens -> the block's branch (the caller adds the shortcut)."""
    w = lambda k: sd[f'{p}.{k}'].to(dt)  # noqa: E731
    C = x.shape[-1]
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w('norm.weight')
    f = F.linear(y, w('fc1.weight'), w('fc1.bias'))
    hidden = f.shape[-1] // 2
    g, i, c = f[..., :hidden], f[..., hidden : 2 * hidden - C], f[..., 2 * hidden - C :]
    if f'{p}.conv.q.weight' in sd:
        c = focused_linear_attention(lambda k: sd[f'{p}.conv.{k}'].to(dt), c, hw)
        c = F.linear(c, w('conv.proj.weight'), w('conv.proj.bias'))
    else:
        cm = c.transpose(1, 2).reshape(c.shape[0], C, *hw)
        c = F.conv2d(cm, w('conv.conv.weight'), w('conv.conv.bias'), padding=3, groups=C).flatten(2).transpose(1, 2)
    return F.linear(F.mish(g) * torch.cat((i, c), dim=-1), w('fc2.weight'), w('fc2.bias'))


def blocks(sd, p, x, dt):
    B, C, H, W = x.shape
    t = x.flatten(2).transpose(1, 2)
    for i in range(seq_len(sd, f'{p}.gated')):
        t = t + gated_block(sd, f'{p}.gated.{i}', t, (H, W), dt)
    return t.transpose(1, 2).reshape(B, C, H, W)


def gater_forward(sd, x):
    dt = x.dtype
    conv = lambda p, t, pad: F.conv2d(t, sd[f'{p}.weight'].to(dt), sd[f'{p}.bias'].to(dt), padding=pad)  # noqa: E731
    down = lambda p, t: F.pixel_unshuffle(conv(f'{p}.body.0', t, 1), 2)  # noqa: E731
    up = lambda p, t: F.pixel_shuffle(conv(f'{p}.body.0', t, 1), 2)  # noqa: E731
    H, W = x.shape[2:]
    xp = F.pad(x, (0, (8 - W % 8) % 8, 0, (8 - H % 8) % 8), mode='reflect')
    e0 = blocks(sd, 'enc0', conv('in_to_dim', xp, 1), dt)
    e1 = blocks(sd, 'enc1.1', down('enc1.0', e0), dt)
    e2 = blocks(sd, 'enc2.1', down('enc2.0', e1), dt)
    lat = up('latent.2', blocks(sd, 'latent.1', down('latent.0', e2), dt))
    d0 = up('dec0.2', blocks(sd, 'dec0.1', conv('dec0.0', torch.cat((lat, e2), 1), 0), dt))
    d1 = up('dec1.2', blocks(sd, 'dec1.1', conv('dec1.0', torch.cat((d0, e1), 1), 0), dt))
    d2 = blocks(sd, 'dec2.0', torch.cat((d1, e0), 1), dt)
    y = conv('dim_to_ch.1', conv('dim_to_ch.0', d2, 1), 1) + xp
    return y[:, :, :H, :W]
