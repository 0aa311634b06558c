"""Plain-PyTorch restatement (in the dtype of the input: fp64 for a high-precision reference) of the FIGSR forward from a state dict (CPU),
written from the layer description in resselt_amd/archs/figsr.  Both transforms of the FourierUnit are the dense matrix DFT of
``resselt_amd.engine.lib_gfisr`` (float64 tables), not ``torch.fft``, as in tests/gfisrv2_oracle.py, whose head this file shares."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from gfisrv2_oracle import head
from mosr_oracle import _conv, _dw

from resselt_amd.engine.lib_gfisr import irfft2_f64, rfft2_f64

MODES = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')
EXTRA = 4


def rms_norm(sd, p, x):
    """x / (eps + ||x||_2 rms) * scale + offset with the checkpoint's own ``eps`` and ``rms`` (figsr/arch.py:406-408)."""
    norm_x = sd[f'{p}.eps'] + x.norm(2, dim=1, keepdim=True) * sd[f'{p}.rms']
    return sd[f'{p}.offset'][:, None, None] + x / norm_x * sd[f'{p}.scale'][:, None, None]


def fourier_unit(sd, p, x):
    b, c, h, w = x.shape
    z = rfft2_f64(x.double()).to(x.dtype)  # [b, c, 2, h, wf]
    z = torch.cat([z[:, :, 0], z[:, :, 1]], 1)  # channels [real of all c | imag of all c]
    z = rms_norm(sd, f'{p}.rn', z)
    z = _dw(z, sd[f'{p}.fpe.weight'], sd[f'{p}.fpe.bias']) + z
    z = F.gelu(F.conv2d(z, sd[f'{p}.fdc.weight'], sd[f'{p}.fdc.bias']))
    z = z.view(b, c, 2, h, -1)  # output channel 2k = real of k, 2k + 1 = imag of k
    y = irfft2_f64(z.double(), h, w).to(x.dtype)
    return rms_norm(sd, f'{p}.post_norm', y)


def _dense(sd, key, x):
    w = sd[f'{key}.weight']
    return F.conv2d(x, w, sd[f'{key}.bias'], padding=(w.shape[2] // 2, w.shape[3] // 2))


def block(sd, b, t):
    dim = t.shape[1]
    hidden = sd[f'{b}.fc2.weight'].shape[1]
    gc = sd[f'{b}.conv.convh.bias'].shape[0]
    f = _conv(sd, f'{b}.fc1', rms_norm(sd, f'{b}.norm', t))
    g, i, c, c_hw, c_w, c_h = torch.split(f, [hidden, hidden - dim, dim - 3 * gc, gc, gc, gc], dim=1)
    parts = [i, fourier_unit(sd, f'{b}.conv.fu', c), _dense(sd, f'{b}.conv.convhw', c_hw), _dense(sd, f'{b}.conv.convw', c_w), _dense(sd, f'{b}.conv.convh', c_h)]
    return _conv(sd, f'{b}.fc2', F.silu(g) * torch.cat(parts, 1)) + t


def figsr_forward(sd, x):
    """``sd``: a FIGSR state dict (``upscale.MetaUpsample`` names the head and the scale); ``x`` [N, 3, H, W]."""
    _, index, scale = (int(v) for v in sd['upscale.MetaUpsample'][:3])
    sd = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith('MetaUpsample')}
    h, w = x.shape[-2:]
    t = (x - sd['shift']) / sd['scale_norm']
    t = F.pad(t, (EXTRA, EXTRA + w % 2, EXTRA, EXTRA + h % 2), mode='reflect')
    t = _conv(sd, 'in_to_dim', t)
    x0, i = t, 0
    while f'gfisr_body_half.{i}.fc1.weight' in sd:
        x0 = block(sd, f'gfisr_body_half.{i}', x0)
        i += 1
    x1, i = x0, 0
    while f'gfisr_body_half_2.{i}.fc1.weight' in sd:
        x1 = block(sd, f'gfisr_body_half_2.{i}', x1)
        i += 1
    x1 = _conv(sd, f'gfisr_body_half_2.{i}', x1)
    y = head(sd, _conv(sd, 'cat_to_dim', torch.cat([x1, t, x0], 1)), MODES[index], scale)
    y = y[:, :, EXTRA * scale : EXTRA * scale + h * scale, EXTRA * scale : EXTRA * scale + w * scale]
    return y * sd['scale_norm'] + sd['shift']
