"""GFISRv2 loader (drop-in for ``resselt/archs/gfisrv2/__init__.py``: the same 22 detection keys, the same inference and metadata).

One deliberate difference in how the module is built, none in what is inferred: the reference hands its module the expansion ratio it
inferred, ``fc1 rows // 2 / dim``, and the module recomputes ``hidden = int(ratio * dim)``; here ``hidden`` is read from the ``fc1`` shape
and handed over beside the ratio, as MoESR's loader does.  A ``pixel_unshuffle`` checkpoint (``in_to_dim.1.weight``) is inferred as the
reference infers it and then refused by the module: the reference cannot load one either.
"""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import GFISRV2, SAMPLE_MODS3

_B = 'gfisr_body.0'
_F = f'{_B}.conv.pconv'
DETECTION_KEYS = (
    f'{_B}.gamma', f'{_B}.norm.scale', f'{_B}.norm.offset', f'{_B}.fc1.weight', f'{_B}.fc1.bias', f'{_F}.rn.scale', f'{_F}.rn.offset',
    f'{_F}.post_norm.scale', f'{_F}.post_norm.offset', f'{_F}.fdc.weight', f'{_F}.fdc.bias', f'{_F}.fpe.weight', f'{_F}.fpe.bias',
    f'{_B}.conv.dwconv_hw.weight', f'{_B}.conv.dwconv_hw.bias', f'{_B}.conv.dwconv_w.weight', f'{_B}.conv.dwconv_w.bias',
    f'{_B}.conv.dwconv_h.weight', f'{_B}.conv.dwconv_h.bias', f'{_B}.fc2.weight', f'{_B}.fc2.bias', 'upscale.MetaUpsample',
)  # fmt: skip


class GFISRV2Arch(Architecture[GFISRV2]):
    def __init__(self):
        super().__init__(uid='GFISRV2', detect=KeyCondition.has_all(*DETECTION_KEYS))

    def load(self, state: Mapping[str, object]) -> GFISRV2:
        _, index, scale, dim, out_ch, mid_dim, _ = (int(v) for v in state['upscale.MetaUpsample'])
        n_blocks = get_seq_len(state, 'gfisr_body') - 3
        hidden = int(state[f'{_B}.fc1.weight'].shape[0]) // 2
        expansion_ratio = hidden / dim
        if 'in_to_dim.weight' in state:
            pixel_unshuffle = False
            in_nc = int(state['in_to_dim.weight'].shape[1])
        else:
            in_nc = int(state['in_to_dim.1.weight'].shape[1])
            in_nc = in_nc // 16 if in_nc % 16 == 0 else in_nc // 4
            pixel_unshuffle = True
        model = GFISRV2(in_nc=in_nc, dim=dim, expansion_ratio=expansion_ratio, scale=scale, out_nc=out_ch, upsampler=SAMPLE_MODS3[index],
                        mid_dim=mid_dim, pixel_unshuffle=pixel_unshuffle, n_blocks=n_blocks, hidden=hidden)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_nc, out_channels=out_ch, upscale=scale, name='GFISRV2')
