"""FlexNet loader (drop-in for ``resselt/archs/flexnet/__init__.py``: the same detection keys, inference rules and metadata).

Documented deviations:
  * ``hidden_rate`` is read from ``t_blocks.0`` of the first LBlock.  The reference reads ``pipeline.att.0.t_blocks.2.ffn.key.weight``
    (``__init__.py:43``) and dies with ``KeyError`` on a linear checkpoint whose first LBlock has fewer than three TransformerBlocks; every
    block has the same ``hidden_rate``, so every checkpoint the reference loads gives the same value here.
  * a ``meta`` pipeline (``pipeline.enc0...``) is detected and refused with ``NotImplementedError``: its U-Net is not built.
  * ``window_size != 8`` is refused with ``NotImplementedError``: the reference itself cannot run it (``LMLTVIT.get_lepe`` hardcodes
    ``H = W = 8``, ``arch.py:174``; 4 and 16 raise a shape error in its ``view``).
"""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import FlexNet


class FlexNetArch(Architecture[FlexNet]):
    def __init__(self):
        super().__init__(
            uid='FlexNet',
            detect=KeyCondition.has_all(
                'short_cut.block.0.weight', 'short_cut.block.0.bias', 'short_cut.block.2.weight', 'short_cut.block.2.bias', 'short_cut.conv11.weight',
                'short_cut.conv11.bias', 'in_to_feat.weight', 'in_to_feat.bias',
                KeyCondition.has_any('pipeline.enc0.0.t_blocks.0.gamma1', 'pipeline.att.0.t_blocks.0.gamma1'),
            ),
        )  # fmt: skip

    def load(self, state: Mapping[str, object]) -> FlexNet:
        if 'pipeline.enc0.0.t_blocks.0.gamma1' in state:
            raise NotImplementedError('FlexNet: the meta pipeline is not built (its U-Net runs the block at up to 8 * dim channels); only the linear pipeline is')
        window_size = int(state['window_size'])
        dim, inp_channels = (int(v) for v in state['in_to_feat.weight'].shape[:2])
        out_channels = inp_channels
        n_lblocks = get_seq_len(state, 'pipeline.att')
        num_blocks = [get_seq_len(state, f'pipeline.att.{i}.t_blocks') for i in range(n_lblocks)]
        hidden, width = (int(v) for v in state['pipeline.att.0.t_blocks.0.ffn.key.weight'].shape)
        hidden_rate = hidden // width
        channel_norm = 'pipeline.att.0.t_blocks.0.ffn.key_norm.weight' in state
        if 'to_img.1.0.weight' in state:
            upsampler = 'n+c'
            scale = int(state['scale_factor'])
            end_index = get_seq_len(state, 'to_img.1') - 1
            out_channels = int(state[f'to_img.1.{end_index}.weight'].shape[0])
        elif 'to_img.init_pos' in state:
            upsampler = 'dys'
            out_channels = int(state['to_img.end_conv.weight'].shape[0])
            scale = math.isqrt(int(state['to_img.offset.weight'].shape[0]) // 8)
        else:
            upsampler = 'ps'
            scale = math.isqrt(int(state['to_img.0.weight'].shape[0]) // out_channels)
        model = FlexNet(inp_channels=inp_channels, out_channels=out_channels, scale=scale, dim=dim, num_blocks=num_blocks, window_size=window_size,
                        hidden_rate=hidden_rate, channel_norm=channel_norm, pipeline_type='linear', upsampler=upsampler)  # fmt: skip
        return self._enhance_model(model=model, in_channels=inp_channels, out_channels=out_channels, upscale=scale, name='FlexNet')
