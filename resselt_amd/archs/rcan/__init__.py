"""RCAN loader (drop-in for ``resselt/archs/rcan/__init__.py``: both detection key sets, the same inferred hyper-parameters and metadata)."""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_pixelshuffle_params, get_seq_len
from .arch import RCAN


class RCANArch(Architecture[RCAN]):
    def __init__(self):
        body = ('tail.1.weight', 'body.0.body.0.body.0.weight', 'body.0.body.0.body.3.conv_du.0.weight')
        super().__init__(
            uid='RCAN',
            detect=KeyCondition.has_any(
                KeyCondition.has_all('head.0.weight', *body),
                KeyCondition.has_all('head.1.weight', *body),  # unshuffle_mod: head.0 is the PixelUnshuffle
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> RCAN:
        n_resgroups = get_seq_len(state_dict, 'body') - 1
        n_resblocks = get_seq_len(state_dict, 'body.0.body') - 1
        scale, n_feats = get_pixelshuffle_params(state_dict, 'tail.0')
        unshuffle_mod = get_seq_len(state_dict, 'head') > 1
        n_colors = state_dict['tail.1.weight'].shape[0]
        head_index = 0
        if unshuffle_mod:
            head_index = 1
            downscale_factor = int(math.sqrt(state_dict['head.1.weight'].shape[1] / n_colors))
            scale = 4 // downscale_factor
        kernel_size = state_dict[f'head.{head_index}.weight'].shape[-1]
        norm = 'sub_mean.weight' in state_dict
        reduction = n_feats // state_dict['body.0.body.0.body.3.conv_du.0.weight'].shape[0]
        # rgb_range, res_scale and act_mode leave no trace in a checkpoint: the reference's fixed values
        model = RCAN(scale=scale, n_resgroups=n_resgroups, n_resblocks=n_resblocks, n_colors=n_colors, rgb_range=255, norm=norm,
                     kernel_size=kernel_size, n_feats=n_feats, reduction=reduction, res_scale=1, act_mode='relu', unshuffle_mod=unshuffle_mod)  # fmt: skip
        return self._enhance_model(model=model, in_channels=n_colors, out_channels=n_colors, upscale=scale, name='RCAN')
