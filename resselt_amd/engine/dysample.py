"""The DySample upsampling head of SPANPlus and RealPLKSR (reference: ``resselt/utilities/dysample.py``) on ``rsa_dysample``.

The offset and scope 1x1 convolutions run as ONE k1 convolution into an f32 map (channels [0, oc) | [oc, 2 oc)).  Bilinear sampling is
linear, so with at most 4 output channels the 1x1 end convolution is applied per channel group BEFORE the sampling, at low resolution
(``zproj``, rsa_dysample's pre-projected mode); wider heads sample the f32 features and apply the end convolution after the sampling.
"""

from __future__ import annotations

import torch

from . import lib as L
from . import ops


def dysample_init_pos(scale: int, groups: int = 4) -> torch.Tensor:
    """The reference's registered buffer (utilities/dysample.py:43-45): sub-pixel centre offsets per group."""
    h = torch.arange((-scale + 1) / 2, (scale - 1) / 2 + 1) / scale
    return torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, groups, 1).reshape(1, -1, 1, 1)


def pack(W: dict, offset_w, offset_b, scope_w, end_w, end_b, init_pos, groups: int, scale: int, **conv) -> None:
    """Pack the head into ``W``: ``end_w`` is [out_ch, C]; ``conv`` goes to ``ConvWeights.from_oihw`` (device, products, fmt)."""
    w = torch.cat([offset_w, scope_w], 0)
    b = torch.cat([offset_b, torch.zeros_like(offset_b)], 0)  # (scope has no bias)
    W['dys.offscope'] = ops.ConvWeights.from_oihw(w, b, **conv)
    out_ch, cin = end_w.shape
    d = dict(init_pos=init_pos.reshape(-1).contiguous(), end_b=end_b.contiguous(), groups=groups, scale=scale, out_ch=out_ch, C=cin, end_w=None)
    if out_ch <= 4:
        # z[4g + o] = sum over the channels c of group g of W_end[o][c] * x[c]
        cpg = cin // groups
        wz = torch.zeros((4 * groups, cin), dtype=torch.float32, device=end_w.device)
        for g in range(groups):
            wz[4 * g : 4 * g + out_ch, g * cpg : (g + 1) * cpg] = end_w[:, g * cpg : (g + 1) * cpg]
        W['dys.zproj'] = ops.ConvWeights.from_oihw(wz[:, :, None, None], None, **conv)
        d['C'] = 4 * groups
    else:
        d['end_w'] = end_w.contiguous()
    W['dys'] = d


def needs_f32_input(W: dict) -> bool:
    """Whether the head samples an f32 map of its input features (the end convolution after the sampling)."""
    return 'dys.zproj' not in W


def emit(plan, W: dict, x, out: torch.Tensor, x_f32: torch.Tensor | None = None) -> None:
    """Emit the head into ``plan``: ``x`` is the input feature planes, ``x_f32`` their f32 map (``needs_f32_input`` only), ``out`` the
    output tensor [N, out_ch, s H, s W]."""
    d = W['dys']
    n, h, w = x.n, x.h, x.w
    G, s = d['groups'], d['scale']
    offscope = plan.f32map(n, 4 * G * s * s, h, w)
    plan.conv(ops.conv_params(W['dys.offscope'], x, h, w, out_f32=offscope))
    if not needs_f32_input(W):
        x_f32 = plan.f32map(n, 4 * G, h, w)
        plan.conv(ops.conv_params(W['dys.zproj'], x, h, w, out_f32=x_f32))
    dp = L.DySampleParams()
    dp.batch, dp.H, dp.W, dp.C, dp.groups, dp.scale, dp.out_ch = n, h, w, d['C'], G, s, d['out_ch']
    dp.x_f32, dp.offscope = x_f32.data_ptr(), offscope.data_ptr()
    dp.init_pos, dp.end_b = d['init_pos'].data_ptr(), d['end_b'].data_ptr()
    dp.end_w = None if d['end_w'] is None else d['end_w'].data_ptr()
    dp.out_nchw, dp.out_dtype = out.data_ptr(), ops.rsa_dtype(out.dtype)
    plan.launch('rsa_dysample', dp)
