"""MoSRv2 loader (drop-in for ``resselt/archs/mosrv2/__init__.py``: same detection, same inferred shapes and metadata).

Documented deviation: a x1 checkpoint with ``unshuffle_mod`` (PixelUnshuffle(4) in front, ``gblocks.1`` reads 48 channels).  The reference
reads the unshuffle factor, 4, as the scale and builds a model without the unshuffle front, whose ``gblocks.0`` is then left at its random
initialisation and whose forward fails on a shape mismatch.  Here the scale is 4 // factor, so such a checkpoint loads as the x1 model it is
(metadata upscale 1).  For the x2 case (factor 2) both readings agree.
"""

from __future__ import annotations

import math
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import SAMPLE_MODS, MoSRv2


def _block_keys(i: int) -> list:
    b = f'gblocks.{i}'
    return [f'{b}.fc1.weight', f'{b}.fc1.bias'] + [f'{b}.conv.{c}.{t}' for c in ('dwconv_hw', 'dwconv_w', 'dwconv_h') for t in ('weight', 'bias')] + [
        f'{b}.fc2.weight', f'{b}.fc2.bias']  # fmt: skip


def _variant(conv: int) -> KeyCondition:
    b = f'gblocks.{conv + 1}'
    return KeyCondition.has_all(
        f'gblocks.{conv}.weight',
        f'gblocks.{conv}.bias',
        f'{b}.gamma',
        KeyCondition.has_any(KeyCondition.has_all(f'{b}.norm.scale', f'{b}.norm.offset'), KeyCondition.has_all(f'{b}.norm.weight', f'{b}.norm.bias')),
        *_block_keys(conv + 1),
        'to_img.MetaUpsample',
        'to_img.0.weight',
        'to_img.0.bias',
    )


class MoSRv2Arch(Architecture[MoSRv2]):
    def __init__(self):
        super().__init__(uid='MoSRv2', detect=KeyCondition.has_any(_variant(1), _variant(0)))

    def load(self, state: Mapping[str, object]) -> MoSRv2:
        _, upsampler, scale, dim, in_ch, mid_dim, _ = [int(i) for i in state['to_img.MetaUpsample']]
        upsampler = SAMPLE_MODS[upsampler]
        n_block = get_seq_len(state, 'gblocks')
        if 'gblocks.0.weight' in state:
            unshuffle_mod = False
            n_block -= 6
            expansion_ratio = state['gblocks.1.fc1.weight'].shape[0] // 2 / dim
            rms_norm = 'gblocks.1.norm.scale' in state
        else:
            unshuffle = math.isqrt(state['gblocks.1.weight'].shape[1] // in_ch)
            scale = 4 // unshuffle  # (the reference: scale = unshuffle; see the module docstring)
            n_block -= 7
            unshuffle_mod = True
            expansion_ratio = state['gblocks.2.fc1.weight'].shape[0] // 2 / dim
            rms_norm = 'gblocks.2.norm.scale' in state
        model = MoSRv2(in_ch=in_ch, scale=scale, n_block=n_block, dim=dim, upsampler=upsampler, expansion_ratio=expansion_ratio, mid_dim=mid_dim,
                       unshuffle_mod=unshuffle_mod, rms_norm=rms_norm)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_ch, out_channels=in_ch, upscale=scale, name='MoSRv2')
