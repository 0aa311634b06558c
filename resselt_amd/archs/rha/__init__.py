"""RHA loader (drop-in for ``resselt/archs/rha/__init__.py``: the same detection keys, inferred hyper-parameters and metadata).

Documented deviation: a checkpoint with an ``unshuffle`` key raises ``NotImplementedError``.  The reference cannot build one either: its
loader divides ``in_ch`` by ``unshuffle ** 2`` twice (``__init__.py:55`` and ``:58``), so a x2 RGB checkpoint (``to_feat.1.weight`` with 12
input channels, unshuffle 2) asks for a module with ``in_ch = 0`` and ``load_state_dict`` fails on the size mismatch of ``to_feat.1.weight``
(run on the CPU against the reference).  The module itself also crops with the internal scale 4 instead of the checkpoint's 2
(``arch.py:565``): the x2 module returns 128 x 128 for a 40 x 40 input.
"""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import RHA, SAMPLE_MODS

_B = 'body.0.body.0'
_OMNI = ('alpha1', 'alpha2', 'alpha3', 'alpha4', 'conv1x1.weight', 'conv1x1.bias', 'conv3x3.weight', 'conv3x3.bias', 'conv5x5.weight', 'conv5x5.bias',
         'conv5x5_reparam.weight', 'conv5x5_reparam.bias')  # fmt: skip
_ATT = ('scale', 'positional_encoding', 'qkv.weight', 'qkv.bias', 'proj.weight', 'proj.bias', 'dwc.weight', 'dwc.bias')


class RHAArch(Architecture[RHA]):
    def __init__(self):
        super().__init__(
            uid='RHA',
            detect=KeyCondition.has_all(
                'body.0.down_sample', f'{_B}.norm.weight', f'{_B}.norm.bias', f'{_B}.fc1.weight', f'{_B}.fc1.bias',
                *(f'{_B}.conv.att.2.{k}' for k in _ATT), *(f'{_B}.conv.conv.{k}' for k in _OMNI),
                f'{_B}.conv.aggr.0.weight', f'{_B}.conv.aggr.0.bias', f'{_B}.fc2.weight', f'{_B}.fc2.bias', 'to_img.MetaUpsample',
            ),
        )  # fmt: skip

    def load(self, state: Mapping[str, object]) -> RHA:
        if 'unshuffle' in state:
            raise NotImplementedError('RHA: checkpoints with unshuffle_mod are not built (the reference loader cannot build them either: see this module\'s docstring)')
        dim, in_ch = (int(v) for v in state['to_feat.weight'].shape[:2])
        group_blocks = get_seq_len(state, 'body')
        res_blocks = get_seq_len(state, 'body.0.body') - 2
        down_list = [int(state[f'body.{i}.down_sample']) for i in range(group_blocks)]
        hidden = int(state[f'{_B}.fc1.weight'].shape[0]) // 2
        _, index, scale, _, out_ch, mid_dim, _ = (int(v) for v in state['to_img.MetaUpsample'])
        window_size = math.isqrt(int(state[f'{_B}.conv.att.2.positional_encoding'].shape[1]))
        model = RHA(dim=dim, scale=scale, in_ch=in_ch, out_ch=out_ch, mid_dim=mid_dim, down_list=down_list, expansion_ratio=hidden / dim, hidden=hidden,
                    group_blocks=group_blocks, res_blocks=res_blocks, upsample=SAMPLE_MODS[index], window_size=window_size)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_ch, out_channels=out_ch, upscale=scale, name='RHA')
