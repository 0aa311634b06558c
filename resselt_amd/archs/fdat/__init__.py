"""FDAT loader (drop-in for ``resselt/archs/fdat/__init__.py``: same detection, same inferred hyper-parameters and metadata).

With ``unshuffle_mod`` the reference reports ``scale = 4 // isqrt(conv_first.1 in-channels / num_out_ch)`` while the module runs its
upsampler at scale 4 (MetaUpsample says 4); the input channel count is taken to be the output channel count, as in the reference.
"""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import FDAT, SAMPLE_MODS3


class FDATArch(Architecture[FDAT]):
    def __init__(self):
        super().__init__(
            uid='FDAT',
            detect=KeyCondition.has_all(
                'groups.0.blocks.0.attn.bias',
                'groups.0.blocks.0.inter.cg.1.weight',
                'groups.0.blocks.0.ffn.fc1.weight',
                'groups.0.blocks.0.n1.weight',
                'upsampler.MetaUpsample',
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> FDAT:
        _, upsampler_index, scale, embed_dim, num_out_ch, mid_dim, _ = [int(v) for v in state_dict['upsampler.MetaUpsample'].tolist()]
        upsampler_type = SAMPLE_MODS3[upsampler_index]
        if 'conv_first.1.weight' in state_dict:
            num_in_ch = num_out_ch
            scale = 4 // math.isqrt(state_dict['conv_first.1.weight'].shape[1] // num_in_ch)
            unshuffle_mod = True
        else:
            unshuffle_mod = False
            num_in_ch = state_dict['conv_first.weight'].shape[1]
        num_groups = get_seq_len(state_dict, 'groups')
        depth_per_group = get_seq_len(state_dict, 'groups.0.blocks') // 2
        bias = state_dict['groups.0.blocks.0.attn.bias']
        num_heads, window_size = bias.shape[0], math.isqrt(bias.shape[2])
        ffn_expansion_ratio = float(state_dict['groups.0.blocks.0.ffn.fc1.weight'].shape[0] / embed_dim)
        aim_reduction_ratio = embed_dim // state_dict['groups.0.blocks.0.inter.cg.1.weight'].shape[0]
        model = FDAT(num_in_ch=num_in_ch, num_out_ch=num_out_ch, scale=scale, embed_dim=embed_dim, num_groups=num_groups, depth_per_group=depth_per_group,
                     num_heads=num_heads, window_size=window_size, ffn_expansion_ratio=ffn_expansion_ratio, aim_reduction_ratio=aim_reduction_ratio,
                     upsampler_type=upsampler_type, mid_dim=mid_dim, img_range=1.0, unshuffle_mod=unshuffle_mod)  # fmt: skip
        return self._enhance_model(model=model, in_channels=num_in_ch, out_channels=num_out_ch, upscale=scale, name='FDAT')
