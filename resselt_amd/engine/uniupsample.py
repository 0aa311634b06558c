"""The UniUpsample heads shared by MoSRv2 (reference ``archs/mosrv2/arch.py:91-172``) and FDAT's UniUpsampleV3 (``archs/fdat/arch.py:291-440``,
its first five modes): conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample.

conv / pixelshuffledirect store through depth-to-space; pixelshuffle (LeakyReLU 0.01) re-lays its shuffled stores out as planes;
nearest+conv reads its x2^n stages through the convolution's nearest-upsample-on-read, and at x3 the convolution before the upsampling is
stored with every output channel repeated 9 times through depth-to-space, which IS the nearest x3 map; dysample is the shared DySample head
(engine/dysample.py) after the optional mid_dim conv + LeakyReLU 0.01.
"""

from __future__ import annotations

import math

import torch

from . import dysample as dys
from . import lib as L
from . import ops

SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')


def head_layers(upsample: str, scale: int, in_dim: int, out_dim: int, mid_dim: int):
    """UniUpsample's layers with parameters: [(index, cout, cin, k)], and the DySample sub-module's index (or None)."""
    if scale == 1 or upsample == 'conv':
        return [(0, out_dim, in_dim, 3)], None
    if upsample == 'pixelshuffledirect':
        return [(0, out_dim * scale * scale, in_dim, 3)], None
    pow2 = scale & (scale - 1) == 0
    if upsample in ('pixelshuffle', 'nearest+conv') and not pow2 and scale != 3:
        raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
    if upsample == 'pixelshuffle':
        layers, i = [(0, mid_dim, in_dim, 3)], 2
        for r in [2] * int(math.log2(scale)) if pow2 else [3]:
            layers.append((i, r * r * mid_dim, mid_dim, 3))
            i += 2
        return layers + [(i, out_dim, mid_dim, 3)], None
    if upsample == 'nearest+conv':
        layers, i = [], 0
        for _ in range(int(math.log2(scale)) if pow2 else 1):
            layers.append((i, in_dim, in_dim, 3))
            i += 3
        return layers + [(i, in_dim, in_dim, 3), (i + 2, out_dim, in_dim, 3)], None
    if upsample == 'dysample':
        if mid_dim != in_dim:
            return [(0, mid_dim, in_dim, 3)], 2
        return [], 0
    raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')


def head_shapes(shapes: dict, buffers: dict, prefix: str, layers, dys_index, scale: int, in_dim: int, out_dim: int, mid_dim: int) -> None:
    """Parameter shapes (and DySample's ``init_pos`` buffer) of a head under ``prefix`` (e.g. 'to_img', 'upsampler')."""
    for i, co, ci, k in layers:
        shapes[f'{prefix}.{i}.weight'] = (co, ci, k, k)
        shapes[f'{prefix}.{i}.bias'] = (co,)
    if dys_index is not None:
        d, s = f'{prefix}.{dys_index}', scale
        dys_dim = mid_dim if dys_index else in_dim
        if dys_dim <= 4 or dys_dim % 4:
            raise ValueError('Incorrect in_channels and groups values.')
        shapes[f'{d}.end_conv.weight'] = (out_dim, dys_dim, 1, 1)
        shapes[f'{d}.end_conv.bias'] = (out_dim,)
        shapes[f'{d}.offset.weight'] = (8 * s * s, dys_dim, 1, 1)
        shapes[f'{d}.offset.bias'] = (8 * s * s,)
        shapes[f'{d}.scope.weight'] = (8 * s * s, dys_dim, 1, 1)
        buffers[f'{d}.init_pos'] = dys.dysample_init_pos(s, 4)


def pack_head(W: dict, sd: dict, prefix: str, upsample: str, scale: int, layers, dys_index, out_dim: int, products, device) -> None:
    """Pack a head's layers into ``W`` as 'head0', 'head1', ... (and DySample's tensors)."""
    cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
    for j, (i, co, ci, k) in enumerate(layers):
        w, b = sd[f'{prefix}.{i}.weight'], sd[f'{prefix}.{i}.bias']
        if upsample == 'nearest+conv' and scale == 3 and j == 0:
            # conv -> Upsample(3): every output channel 9 times, stored through depth-to-space (channel 9c + k -> sub-pixel k of c)
            w, b = w.repeat_interleave(9, 0), b.repeat_interleave(9, 0)
        W[f'head{j}'] = cw(w, b)
    if dys_index is not None:
        d = f'{prefix}.{dys_index}'
        dys.pack(W, sd[f'{d}.offset.weight'], sd[f'{d}.offset.bias'], sd[f'{d}.scope.weight'], sd[f'{d}.end_conv.weight'].reshape(out_dim, -1),
                 sd[f'{d}.end_conv.bias'], sd[f'{d}.init_pos'], 4, scale, products=products, device=device)  # fmt: skip


def needs_f32_input(upsample: str, scale: int, dys_index, W: dict) -> bool:
    """Whether ``emit_head`` reads an f32 map of the head's input (DySample sampling the input features themselves)."""
    return scale != 1 and upsample == 'dysample' and dys_index == 0 and dys.needs_f32_input(W)


def emit_head(plan, W: dict, upsample: str, s: int, layers, dim: int, mid_dim: int, dys_index, fe, fe32, y, n: int, H: int, Wd: int,
              with_lo: bool) -> None:  # noqa: C901  (fmt: skip)
    """Emit the head from the feature planes ``fe`` (``dim`` channels, H x Wd; ``fe32`` its f32 map when ``needs_f32_input``) into the
    output tensor ``y`` [n, out, s H, s Wd]."""
    if s == 1 or upsample in ('conv', 'pixelshuffledirect'):
        plan.conv(ops.conv_params(W['head0'], fe, H, Wd, out_nchw=y, pixel_shuffle=1 if upsample == 'conv' or s == 1 else s))
        return
    if upsample == 'dysample':
        x, x32 = fe, fe32
        if dys_index == 2:
            x = plan.planes(n, mid_dim // 8, H, Wd, with_lo)
            x32 = plan.f32map(n, mid_dim, H, Wd) if dys.needs_f32_input(W) else None
            plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.01, out=x, out_f32=x32))
        dys.emit(plan, W, x, y, x32)
        return
    if upsample == 'pixelshuffle':
        mid = mid_dim
        t = plan.planes(n, mid // 8, H, Wd, with_lo)
        plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.01, out=t))
        hh, ww = H, Wd
        for j in range(1, len(layers) - 1):
            r = math.isqrt(layers[j][1] // mid)
            shuffled = torch.empty((n, mid, hh * r, ww * r), dtype=torch.float32, device=plan.device)
            plan.keep.append(shuffled)
            plan.conv(ops.conv_params(W[f'head{j}'], t, hh, ww, out_nchw=shuffled, pixel_shuffle=r))
            hh, ww = hh * r, ww * r
            t = plan.planes(n, mid // 8, hh, ww, with_lo)
            plan.call(lambda src=shuffled, dst=t: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
        plan.conv(ops.conv_params(W[f'head{len(layers) - 1}'], t, hh, ww, out_nchw=y))
        return
    # nearest+conv: conv -> Upsample -> LeakyReLU(0.2) per stage (the activation commutes with the nearest upsampling)
    pd = (dim + 7) // 8
    t, hh, ww = fe, H, Wd
    stages = len(layers) - 2
    upsampled = False
    if s == 3:
        shuffled = torch.empty((n, dim, 3 * H, 3 * Wd), dtype=torch.float32, device=plan.device)
        plan.keep.append(shuffled)
        plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.2, out_nchw=shuffled, pixel_shuffle=3))
        hh, ww = 3 * H, 3 * Wd
        t = plan.planes(n, pd, hh, ww, with_lo)
        plan.call(lambda src=shuffled, dst=t: ops.nchw_to_planes(src, dst))
        plan.count_launches(1)
    else:
        for j in range(stages):
            o = plan.planes(n, pd, hh * 2 if upsampled else hh, ww * 2 if upsampled else ww, with_lo)
            if upsampled:
                hh, ww = hh * 2, ww * 2
            plan.conv(ops.conv_params(W[f'head{j}'], t, hh, ww, upsample2x=upsampled, act=L.ACT_LRELU, act_param=0.2, out=o))
            t, upsampled = o, True
    if upsampled:
        hh, ww = hh * 2, ww * 2
    o = plan.planes(n, pd, hh, ww, with_lo)
    plan.conv(ops.conv_params(W[f'head{stages}'], t, hh, ww, upsample2x=upsampled, act=L.ACT_LRELU, act_param=0.2, out=o))
    plan.conv(ops.conv_params(W[f'head{stages + 1}'], o, hh, ww, out_nchw=y))
