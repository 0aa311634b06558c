"""ATD loader (drop-in for ``resselt/archs/atd/__init__.py``: same detection, same inferred hyper-parameters, tags and metadata)."""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_pixelshuffle_params, get_seq_len, pixelshuffle_scale
from .arch import ATD

_L0 = 'layers.0.residual_group.layers.0'


class ATDArch(Architecture[ATD]):
    def __init__(self):
        super().__init__(
            uid='ATD',
            detect=KeyCondition.has_all(
                'relative_position_index_SA',
                'conv_first.weight',
                'conv_first.bias',
                'layers.0.residual_group.td',
                f'{_L0}.sigma',
                f'{_L0}.norm1.weight',
                f'{_L0}.norm1.bias',
                f'{_L0}.norm2.weight',
                f'{_L0}.norm2.bias',
                f'{_L0}.norm3.weight',
                f'{_L0}.norm3.bias',
                f'{_L0}.wqkv.weight',
                f'{_L0}.attn_win.relative_position_bias_table',
                f'{_L0}.attn_win.proj.weight',
                f'{_L0}.attn_win.proj.bias',
                f'{_L0}.attn_atd.scale',
                f'{_L0}.attn_atd.wq.weight',
                f'{_L0}.attn_atd.wk.weight',
                f'{_L0}.attn_atd.wv.weight',
                f'{_L0}.attn_aca.logit_scale',
                f'{_L0}.attn_aca.proj.weight',
                f'{_L0}.convffn.fc1.weight',
                f'{_L0}.convffn.fc1.bias',
                f'{_L0}.convffn.dwconv.depthwise_conv.0.weight',
                f'{_L0}.convffn.dwconv.depthwise_conv.0.bias',
                f'{_L0}.convffn.fc2.weight',
                f'{_L0}.convffn.fc2.bias',
                'norm.weight',
                'norm.bias',
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> ATD:
        sd = state_dict
        in_chans = sd['conv_first.weight'].shape[1]
        embed_dim = sd['conv_first.weight'].shape[0]
        window_size = math.isqrt(sd['relative_position_index_SA'].shape[0])
        num_layers = get_seq_len(sd, 'layers')
        depths = [get_seq_len(sd, f'layers.{i}.residual_group.layers') for i in range(num_layers)]
        num_heads = [sd[f'layers.{i}.residual_group.layers.0.attn_win.relative_position_bias_table'].shape[1] for i in range(num_layers)]
        num_tokens = sd[f'{_L0}.attn_atd.scale'].shape[0]
        reducted_dim = sd[f'{_L0}.attn_atd.wq.weight'].shape[0]
        convffn_kernel_size = sd[f'{_L0}.convffn.dwconv.depthwise_conv.0.weight'].shape[2]
        mlp_ratio = sd[f'{_L0}.convffn.fc1.weight'].shape[0] / embed_dim
        qkv_bias = f'{_L0}.wqkv.bias' in sd
        ape = 'absolute_pos_embed' in sd
        patch_norm = 'patch_embed.norm.weight' in sd
        resi_connection = '1conv' if 'layers.0.conv.weight' in sd else '3conv'
        if 'conv_up1.weight' in sd:
            upsampler, upscale = 'nearest+conv', 4
        elif 'conv_before_upsample.0.weight' in sd:
            upsampler = 'pixelshuffle'
            upscale, _ = get_pixelshuffle_params(sd, 'upsample')
        elif 'conv_last.weight' in sd:
            upsampler, upscale = '', 1
        else:
            upsampler = 'pixelshuffledirect'
            upscale = pixelshuffle_scale(sd['upsample.0.weight'].shape[0], in_chans)
        norm = 'no_norm' not in sd
        is_light = upsampler == 'pixelshuffledirect' and embed_dim == 48
        category_size = 128 if is_light else 256  # the reference's heuristic
        tags = [f'{embed_dim}dim', f'{window_size}w', f'{category_size}cat']
        if is_light:
            tags.insert(0, 'light')
        model = ATD(img_size=64, patch_size=1, in_chans=in_chans, embed_dim=embed_dim, depths=depths, num_heads=num_heads, window_size=window_size,
                    category_size=category_size, num_tokens=num_tokens, reducted_dim=reducted_dim, convffn_kernel_size=convffn_kernel_size,
                    mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, ape=ape, patch_norm=patch_norm, upscale=upscale, img_range=1.0, upsampler=upsampler,
                    resi_connection=resi_connection, norm=norm)  # fmt: skip
        model.tags = tags
        return self._enhance_model(model=model, in_channels=in_chans, out_channels=in_chans, upscale=upscale, name='ATD')
