"""Oracle for Real-CUGAN (TEST INFRASTRUCTURE, see oracle/__init__.py).

Functional fp32 restatement of ``resselt/archs/cugan/arch.py`` (UpCunet2x / 3x / 4x / 2x_fast, ``alpha = 1``) over the checkpoint's own
key names, on whole tensors: a real reflect ``F.pad``, valid convolutions, negative-pad crops and SE means over the whole map.  Shape
errors come from torch itself, so the oracle raises wherever the reference does (a reflect pad not smaller than the input, U-Net maps
that do not line up) -- also on the ``meta`` device, where it costs nothing (tests/test_cugan_geometry.py).  Pinned by
tests/golden/cugan_*.npz (outputs of the reference itself).
"""

from __future__ import annotations

from typing import Mapping

import torch
import torch.nn.functional as F

PRO_SCALE, PRO_SHIFT = 0.7, 0.15  # arch.py:305, 318 (and the 3x / 4x copies)


def cugan_variant(sd: Mapping[str, torch.Tensor]) -> str:
    """What CUGANArch.load infers (resselt/archs/cugan/__init__.py:50-72)."""
    if 'conv_final.weight' in sd:
        return '2x_fast' if sd['unet1.conv1.conv.0.weight'].shape[1] == 12 else '4x'
    return '3x' if sd['unet1.conv_bottom.weight'].shape[2] == 5 else '2x'


def _conv(sd, key, x, stride=1):
    return F.conv2d(x, sd[f'{key}.weight'], sd[f'{key}.bias'], stride=stride)


def _lrelu(x):
    return F.leaky_relu(x, 0.1)


def _crop(x, k):
    """F.pad(x, (-k, -k, -k, -k)) (arch.py:124, 233, 237, 312)."""
    return F.pad(x, (-k, -k, -k, -k))


def se_block(sd, key, x):
    """SEBlock.forward (arch.py:57-67): a sigmoid gate from the mean over the whole map."""
    s = x.mean(dim=(2, 3), keepdim=True)
    s = torch.sigmoid(_conv(sd, f'{key}.conv2', F.relu(_conv(sd, f'{key}.conv1', s))))
    return x * s


def unet_conv(sd, key, x, se):
    """UNetConv.forward (arch.py:78-96): two valid 3x3 convolutions with LeakyReLU(0.1), then SE."""
    z = _lrelu(_conv(sd, f'{key}.conv.2', _lrelu(_conv(sd, f'{key}.conv.0', x))))
    return se_block(sd, f'{key}.seblock', z) if se else z


def unet1(sd, x, bottom):
    """UNet1.forward / UNet1x3.forward (arch.py:121-132, 173-184); ``bottom`` = (stride, padding) of the transposed tail."""
    x1 = unet_conv(sd, 'unet1.conv1', x, False)
    x2 = _lrelu(_conv(sd, 'unet1.conv1_down', x1, stride=2))
    x1 = _crop(x1, 4)
    x2 = unet_conv(sd, 'unet1.conv2', x2, True)
    x2 = _lrelu(F.conv_transpose2d(x2, sd['unet1.conv2_up.weight'], sd['unet1.conv2_up.bias'], stride=2))
    x3 = _lrelu(_conv(sd, 'unet1.conv3', x1 + x2))
    stride, pad = bottom
    return F.conv_transpose2d(x3, sd['unet1.conv_bottom.weight'], sd['unet1.conv_bottom.bias'], stride=stride, padding=pad)


def unet2(sd, x):
    """UNet2.forward (arch.py:230-249), alpha = 1, with a 3x3 valid convolution tail (deconv=False)."""
    x1 = unet_conv(sd, 'unet2.conv1', x, False)
    x2 = _lrelu(_conv(sd, 'unet2.conv1_down', x1, stride=2))
    x1 = _crop(x1, 16)
    x2 = unet_conv(sd, 'unet2.conv2', x2, True)
    x3 = _lrelu(_conv(sd, 'unet2.conv2_down', x2, stride=2))
    x2 = _crop(x2, 4)
    x3 = unet_conv(sd, 'unet2.conv3', x3, True)
    x3 = _lrelu(F.conv_transpose2d(x3, sd['unet2.conv3_up.weight'], sd['unet2.conv3_up.bias'], stride=2))
    x4 = unet_conv(sd, 'unet2.conv4', x2 + x3, True)
    x4 = _lrelu(F.conv_transpose2d(x4, sd['unet2.conv4_up.weight'], sd['unet2.conv4_up.bias'], stride=2))
    x5 = _lrelu(_conv(sd, 'unet2.conv5', x1 + x4))
    return _conv(sd, 'unet2.conv_bottom', x5)


# variant -> (reflect pad, multiple the padded size is rounded up to, scale, unet1 tail (stride, padding))
_GEOM = {'2x': (18, 2, 2, (2, 3)), '3x': (14, 4, 3, (3, 2)), '4x': (19, 2, 4, (2, 3)), '2x_fast': (38, 2, 2, (2, 3))}


def cugan_forward(sd: Mapping[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """UpCunet2x.forward (arch.py:300-320), UpCunet3x.forward (341-361), UpCunet4x.forward (384-413), UpCunet2x_fast.forward (427-444)."""
    variant = cugan_variant(sd)
    pro = 'pro' in sd
    pad, mult, scale, bottom = _GEOM[variant]
    _, _, h0, w0 = x.shape
    if pro:
        x = x * PRO_SCALE + PRO_SHIFT
    x00 = x
    ph = ((h0 - 1) // mult + 1) * mult
    pw = ((w0 - 1) // mult + 1) * mult
    x = F.pad(x, (pad, pad + pw - w0, pad, pad + ph - h0), 'reflect')
    if variant == '2x_fast':
        x = F.pixel_unshuffle(x, 2)
    x = unet1(sd, x, bottom)
    x = unet2(sd, x) + _crop(x, 20)
    if variant in ('4x', '2x_fast'):
        x = F.pixel_shuffle(_crop(_conv(sd, 'conv_final', x), 1), 2)
    if w0 != pw or h0 != ph:
        x = x[:, :, : h0 * scale, : w0 * scale]
    if variant in ('4x', '2x_fast'):
        x = x + F.interpolate(x00, scale_factor=scale, mode='nearest')
    if pro:
        x = (x - PRO_SHIFT) / PRO_SCALE
    return x
