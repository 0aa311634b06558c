"""SMoSR loader (drop-in for ``resselt/archs/smosr/__init__.py``: the same detection keys, the same inference and metadata).

``dim`` and ``in_ch`` come from the shape of ``blocks_1.0.body.0.eval_conv.weight`` -- the only use of an ``eval_conv`` tensor: their
values are never read -- ``n_mb`` from the length of ``blocks_2``, the rest from the ``upsampler.MetaUpsample`` uint8 buffer, and DySample's
end kernel from ``upsampler.2.end_conv.weight``.
"""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import SAMPLE_MODS, SMoSR

_BODIES = tuple(f'{b}.body.{i}.eval_conv.{t}' for b in ('blocks_1.0', 'blocks_1.1', 'blocks_2.0', 'end_block.0') for i in (0, 2, 4) for t in ('weight', 'bias'))
DETECTION_KEYS = (
    ('short.weight', 'short.bias', 'blocks_1.0.short.weight', 'blocks_1.0.short.bias') + _BODIES
    + ('end_block.1.eval_conv.weight', 'end_block.1.eval_conv.bias', 'upsampler.MetaUpsample')
)  # fmt: skip


class SMoSRArch(Architecture[SMoSR]):
    def __init__(self):
        super().__init__(uid='SMoSR', detect=KeyCondition.has_all(*DETECTION_KEYS))

    def load(self, state: Mapping[str, object]) -> SMoSR:
        dim, in_ch = (int(v) for v in state['blocks_1.0.body.0.eval_conv.weight'].shape[:2])
        n_mb = get_seq_len(state, 'blocks_2')
        _, index, scale, _, out_dim, mid_dim, _, rep = (int(v) for v in state['upsampler.MetaUpsample'])
        d_kernel = 1
        if index == SAMPLE_MODS.index('dysample'):
            if 'upsampler.2.end_conv.weight' not in state and scale != 1:
                raise NotImplementedError('SMoSR: the dysample head with mid_dim == dim + in_ch * scale^2 is not built: the reference\'s loader '
                                          'raises KeyError on upsampler.2.end_conv.weight')  # fmt: skip
            if 'upsampler.2.end_conv.weight' in state:
                d_kernel = int(state['upsampler.2.end_conv.weight'].shape[2])
        model = SMoSR(in_ch=in_ch, out_ch=out_dim, dim=dim, scale=scale, rep=bool(rep), n_mb=n_mb, upsampler=SAMPLE_MODS[index],
                      upsampler_mid_dim=mid_dim, d_kernel=d_kernel)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_ch, out_channels=out_dim, upscale=scale, name='SMoSR')
