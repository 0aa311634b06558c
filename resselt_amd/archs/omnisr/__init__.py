"""OmniSR loader (drop-in for ``resselt/archs/omni/__init__.py``: same detection, junk-key removal, inferred hyper-parameters and metadata)."""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len, pixelshuffle_scale
from .arch import OmniSR


class OmniSRArch(Architecture[OmniSR]):
    def __init__(self):
        super().__init__(
            uid='OmniSR',
            detect=KeyCondition.has_all(
                'residual_layer.0.residual_layer.0.layer.0.fn.0.weight',
                'input.weight',
                'up.0.weight',
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> OmniSR:
        # as the reference: profiler counters (thop) are deleted from the mapping it is given
        for key in list(state_dict.keys()):
            if key.endswith(('total_ops', 'total_params')):
                del state_dict[key]
        window_size = 8
        num_feat, num_in_ch = state_dict['input.weight'].shape[:2]
        num_out_ch = num_in_ch
        bias = 'input.bias' in state_dict
        up_scale = pixelshuffle_scale(state_dict['up.0.weight'].shape[0], num_in_ch)
        res_num = get_seq_len(state_dict, 'residual_layer')
        block_num = get_seq_len(state_dict, 'residual_layer.0.residual_layer') - 1
        rel_pos_bias_key = 'residual_layer.0.residual_layer.0.layer.2.fn.rel_pos_bias.weight'
        pe = rel_pos_bias_key in state_dict
        if pe:
            window_size = int((math.sqrt(state_dict[rel_pos_bias_key].shape[0]) + 1) / 2)
        model = OmniSR(num_in_ch=num_in_ch, num_out_ch=num_out_ch, num_feat=num_feat, block_num=block_num, pe=pe, window_size=window_size,
                       res_num=res_num, up_scale=up_scale, bias=bias)  # fmt: skip
        return self._enhance_model(model=model, in_channels=num_in_ch, out_channels=num_out_ch, upscale=up_scale, name='OmniSR')
