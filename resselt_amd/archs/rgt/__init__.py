"""RGT loader (drop-in for ``resselt/archs/rgt/__init__.py``: same detection, same inferred hyper-parameters and metadata)."""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_pixelshuffle_params, get_seq_len
from .arch import RGT


def _get_split_size(state_dict: Mapping[str, object]) -> tuple[int, int]:
    """split_size from the sizes of the first window's index and bias table.  Only a square split is determined uniquely; otherwise the
    reference assumes split[0] <= split[1], both powers of two."""
    a = state_dict['layers.0.blocks.0.attn.attns.0.relative_position_index'].shape[0]
    b = state_dict['layers.0.blocks.0.attn.attns.0.rpe_biases'].shape[0]

    def is_solution(ssw: int, ssh: int) -> bool:
        return ssw * ssh == a and (2 * ssw - 1) * (2 * ssh - 1) == b

    square = math.isqrt(a)
    if is_solution(square, square):
        return square, square
    for i in range(1, 10):
        for j in range(i + 1, 10):
            if is_solution(2**i, 2**j):
                return 2**i, 2**j
    raise ValueError(f'No valid split_size found for {a=} and {b=}')


class RGTArch(Architecture[RGT]):
    def __init__(self):
        super().__init__(
            uid='RGT',
            detect=KeyCondition.has_all(
                'conv_first.weight',
                'before_RG.1.weight',
                'layers.0.blocks.0.gamma',
                'layers.0.blocks.0.norm1.weight',
                'layers.0.blocks.0.attn.qkv.weight',
                'layers.0.blocks.0.attn.proj.weight',
                'layers.0.blocks.0.attn.attns.0.rpe_biases',
                'layers.0.blocks.0.attn.attns.0.relative_position_index',
                'layers.0.blocks.0.attn.attns.0.pos.pos_proj.weight',
                'layers.0.blocks.0.mlp.fc1.weight',
                'layers.0.blocks.0.mlp.fc2.weight',
                'layers.0.blocks.0.norm2.weight',
                'norm.weight',
                KeyCondition.has_any('conv_after_body.weight', 'conv_after_body.0.weight'),
                'conv_before_upsample.0.weight',
                'conv_last.weight',
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> RGT:
        sd = state_dict
        in_chans = sd['conv_first.weight'].shape[1]
        embed_dim = sd['conv_first.weight'].shape[0]
        num_layers = get_seq_len(sd, 'layers')
        depth = [get_seq_len(sd, f'layers.{i}.blocks') for i in range(num_layers)]
        num_heads = []
        for i in range(num_layers):
            heads_half = sd[f'layers.{i}.blocks.0.attn.attns.0.pos.pos3.2.weight'].shape[0]
            num_heads.append(heads_half * 2 if embed_dim % (heads_half * 2) == 0 else heads_half * 2 + 1)
        qkv_bias = 'layers.0.blocks.0.attn.qkv.bias' in sd
        w1 = sd['layers.0.blocks.0.mlp.fc1.weight']
        mlp_ratio = w1.shape[0] / w1.shape[1]
        resi_connection = '1conv' if 'conv_after_body.weight' in sd else '3conv'
        c_ratio = 0.5  # only defined if some group has a second block
        for i, d in enumerate(depth):
            if d >= 2:
                w = sd[f'layers.{i}.blocks.1.attn.conv.weight']
                c_ratio = w.shape[0] / w.shape[1]
                break
        upscale, _ = get_pixelshuffle_params(sd, 'upsample')
        split_size = _get_split_size(sd)
        model = RGT(img_size=64, in_chans=in_chans, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                    upscale=upscale, img_range=1.0, resi_connection=resi_connection, split_size=split_size, c_ratio=c_ratio)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_chans, out_channels=in_chans, upscale=upscale, name='RGT')
