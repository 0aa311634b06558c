"""Plain-PyTorch restatement (in the dtype of the input: fp32, or fp64 for a high-precision reference) of the MoESR forward from a state dict
(CPU), written from the layer description in resselt_amd/archs/moesr.  The gated block and the UniUpsample heads are mosr_oracle.py's."""

from __future__ import annotations

import torch
import torch.nn.functional as F

from mosr_oracle import _conv, _dw, _gated, _head, _layer_norm

SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')


def _block(sd, b, t):
    hidden = sd[f'{b}.fc2.weight'].shape[1]
    gc = sd[f'{b}.conv.dwconv_hw.weight'].shape[0]

    def conv_fn(rest):
        i_id = hidden - 3 * gc
        parts = [rest[:, :i_id]]
        for j, name in enumerate(('dwconv_hw', 'dwconv_w', 'dwconv_h')):
            parts.append(_dw(rest[:, i_id + j * gc : i_id + (j + 1) * gc], sd[f'{b}.conv.{name}.weight'], sd[f'{b}.conv.{name}.bias']))
        return torch.cat(parts, 1)

    n = _layer_norm(t, sd[f'{b}.norm.weight'], sd[f'{b}.norm.bias'])
    return _gated(sd, b, n, hidden, conv_fn) * sd[f'{b}.gamma'] + t


def _blocks(sd, prefix, t):
    j = 0
    while f'{prefix}.{j}.fc1.weight' in sd:
        t = _block(sd, f'{prefix}.{j}', t)
        j += 1
    return t


def moesr_forward(sd, x):
    """The head's mode, scale and mid width are read from ``upscale.MetaUpsample``, as the reference's loader reads them."""
    _, index, scale, _, _, mid_dim, _ = (int(v) for v in sd['upscale.MetaUpsample'])
    sd = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith('MetaUpsample')}
    _, _, h, w = x.shape
    ph, pw = h % 2, w % 2
    xp = F.pad(x, (0, pw, 0, ph), 'reflect') if (ph or pw) else x
    trunk = _conv(sd, 'in_to_dim', xp)
    t, g = trunk, 0
    while f'blocks.{g}.msg.down.0.weight' in sd:
        t = _blocks(sd, f'blocks.{g}.blocks', t)
        m = f'blocks.{g}.msg'
        d = F.leaky_relu(F.pixel_unshuffle(_conv(sd, f'{m}.down.0', t), 2), 0.1)
        d = _blocks(sd, f'{m}.gated', d)
        t = F.leaky_relu(F.pixel_shuffle(_conv(sd, f'{m}.up.0', d), 2), 0.1) + t
        g += 1
    t = t + trunk
    head = {k.replace('upscale.', 'to_img.', 1): v for k, v in sd.items() if k.startswith('upscale.')}
    y = _head(head, t, SAMPLE_MODS[index], scale, mid_dim)
    return y[:, :, : h * scale, : w * scale]
