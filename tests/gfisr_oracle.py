"""Plain-PyTorch restatement (in the dtype of the input: fp64 for a high-precision reference) of the GFISR (v1) forward from a state dict
(CPU), eval-mode semantics, written from the layer description in resselt_amd/archs/gfisr.  Both transforms of the FourierUnit are the dense
matrix DFT of ``resselt_amd.engine.lib_gfisr`` (float64 tables) around an explicit ``F.pad(..., 'reflect')`` and crop; the spectral
channels are handled in the reference's interleaved (re, im) order, so the pack-time permutation of the engine is checked, not repeated."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from gfisrv2_oracle import head
from mosr_oracle import _conv, _dw, _layer_norm

from resselt_amd.engine.lib_gfisr import irfft2_f64, rfft2_f64

KINDS = ('identity', 'dwconv', 'dwconv', 'dwconv', 'fourier')  # the five Inception modules before rotation
SLOTS = ('pconv', 'dwconv_hw', 'dwconv_w', 'dwconv_h', 'fsas')


def fourier_unit(sd, p, x):
    H, W = x.shape[-2:]
    x = F.pad(x, (2, 2 + W % 2, 2, 2 + H % 2), mode='reflect')  # raises where the reference's pad does
    b, c, h, w = x.shape
    z = rfft2_f64(x.double()).to(x.dtype)  # [b, c, 2, h, wf]
    z = z.reshape(b, 2 * c, h, -1)  # 'b c h w d -> b (c d) h w': channel 2k = real of k, 2k + 1 = imag of k
    z = _layer_norm(z, sd[f'{p}.ln.weight'], sd[f'{p}.ln.bias'])
    z = _dw(z, sd[f'{p}.fpe.weight'], sd[f'{p}.fpe.bias']) + z
    dy = torch.softmax(F.conv2d(z, sd[f'{p}.weight.0.weight'], sd[f'{p}.weight.0.bias']), 1)  # one channel: exactly 1
    z = F.gelu(F.conv2d(z, sd[f'{p}.fdc.weight'], sd[f'{p}.fdc.bias']) * dy)
    y = irfft2_f64(z.view(b, c, 2, h, -1).double(), h, w).to(x.dtype)
    return y[:, :, 2 : 2 + H, 2 : 2 + W]


def block(sd, b, t, shift):
    dim = t.shape[1]
    hidden = sd[f'{b}.fc2.weight'].shape[1]
    gc = dim // 8
    widths = [dim - 4 * gc, gc, gc, gc, gc]
    f = _conv(sd, f'{b}.fc1', _layer_norm(t, sd[f'{b}.norm.weight'], sd[f'{b}.norm.bias']))
    g, i, c = f[:, :hidden], f[:, hidden : 2 * hidden - dim], f[:, 2 * hidden - dim :]
    parts, s0 = [i], 0
    for slot in range(5):
        k = (shift + slot) % 5
        piece, p = c[:, s0 : s0 + widths[k]], f'{b}.conv.{SLOTS[slot]}'
        if KINDS[k] == 'fourier' and f'{p}.ln.weight' in sd:
            parts.append(fourier_unit(sd, p, piece))
        elif KINDS[k] == 'dwconv':
            parts.append(_dw(piece, sd[f'{p}.weight'], sd[f'{p}.bias']))
        else:  # the identity, and the fifth module with fft_mode=False
            parts.append(piece)
        s0 += widths[k]
    return F.mish(_conv(sd, f'{b}.fc2', F.mish(g) * torch.cat(parts, 1))) * sd[f'{b}.gamma'] + t


def gfisr_forward(sd, x, scale=None):
    """``sd``: a GFISR state dict (``dim_to_out.MetaUpsample`` names the head and its scale); ``x`` [N, C, H, W].  ``scale``: the model's
    scale where it is not the head's (a ``pixel_unshuffle`` model: ``in_to_dim.1`` in the keys, head at 4)."""
    modes = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')
    _, index, s_head = (int(v) for v in sd['dim_to_out.MetaUpsample'][:3])
    sd = {k.replace('dim_to_out.', 'upscale.'): v.to(x.dtype) for k, v in sd.items() if not k.endswith('MetaUpsample')}
    h, w = x.shape[-2:]
    if 'in_to_dim.1.weight' in sd:
        u = 4 // scale
        xp = F.pad(x, (0, (u - w % u) % u, 0, (u - h % u) % u), 'reflect')
        t0 = _conv(sd, 'in_to_dim.1', F.pixel_unshuffle(xp, u))
    else:
        scale = s_head
        t0 = _conv(sd, 'in_to_dim', x)
    t, i = t0, 0
    while f'net.{i}.fc1.weight' in sd:
        t = block(sd, f'net.{i}', t, i)
        i += 1
    return head(sd, t + t0, modes[index], s_head)[:, :, : h * scale, : w * scale]
