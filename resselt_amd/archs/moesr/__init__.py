"""MoESR loader (drop-in for ``resselt/archs/moesr/__init__.py``: the same sixteen detection keys, the same inference and metadata).

One deliberate difference in how the module is built, none in what is inferred: the reference hands its module the expansion ratios it
inferred, ``(fc1 rows / fc1 columns) / 2``, and the module recomputes ``hidden = int(ratio * dim)`` -- which can be off by one from the
checkpoint's own ``hidden`` for a ratio that is no binary fraction.  Here the two hidden widths are read from the ``fc1`` shapes and handed
over beside the ratios.
"""

from __future__ import annotations

from typing import Mapping

from ...engine.uniupsample import SAMPLE_MODS
from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import MoESR

_B = 'blocks.0.blocks.0'
DETECTION_KEYS = (
    'in_to_dim.weight', 'in_to_dim.bias', f'{_B}.gamma', f'{_B}.norm.weight', f'{_B}.norm.bias', f'{_B}.fc1.weight', f'{_B}.fc1.bias',
    f'{_B}.conv.dwconv_hw.weight', f'{_B}.conv.dwconv_hw.bias', f'{_B}.conv.dwconv_w.weight', f'{_B}.conv.dwconv_w.bias',
    f'{_B}.conv.dwconv_h.weight', f'{_B}.conv.dwconv_h.bias', f'{_B}.fc2.weight', f'{_B}.fc2.bias', 'upscale.MetaUpsample',
)  # fmt: skip


class MoESRArch(Architecture[MoESR]):
    def __init__(self):
        super().__init__(uid='MoESR', detect=KeyCondition.has_all(*DETECTION_KEYS))

    def load(self, state: Mapping[str, object]) -> MoESR:
        dim, in_ch = (int(v) for v in state['in_to_dim.weight'].shape[:2])
        n_blocks = get_seq_len(state, 'blocks')
        n_block = get_seq_len(state, 'blocks.0.blocks')
        fc1 = state[f'{_B}.fc1.weight'].shape
        fc1_msg = state['blocks.0.msg.gated.0.fc1.weight'].shape
        expansion_factor = (fc1[0] / fc1[1]) / 2
        expansion_msg = (fc1_msg[0] / fc1_msg[1]) / 2
        _, index, scale, _, out_ch, upsample_dim, _ = (int(v) for v in state['upscale.MetaUpsample'])
        model = MoESR(in_ch=in_ch, out_ch=out_ch, scale=scale, dim=dim, n_blocks=n_blocks, n_block=n_block, expansion_factor=expansion_factor,
                      expansion_msg=expansion_msg, upsampler=SAMPLE_MODS[index], upsample_dim=upsample_dim, hidden=int(fc1[0]) // 2,
                      hidden_msg=int(fc1_msg[0]) // 2)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_ch, out_channels=out_ch, upscale=scale, name='MoESR')
