"""GateR loader (drop-in for ``resselt/archs/gater/__init__.py``: same detection key set, same inferred shapes and metadata)."""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import BLOCK_LIST, GateR


def _detect_keys() -> list[str]:
    """in_to_dim, dim_to_ch, every level's first block (norm.weight, fc1, fc2 -- and the depthwise ``conv.conv`` everywhere but in the latent
    stage, which a ``latent_att`` checkpoint fills with the attention instead), the three Downsample / Upsample convolutions and the two 1x1
    convolutions in front of dec0 and dec1."""
    keys = []
    for name in ('in_to_dim', 'dim_to_ch.0', 'dim_to_ch.1', 'enc1.0.body.0', 'enc2.0.body.0', 'latent.0.body.0', 'latent.2.body.0', 'dec0.0', 'dec0.2.body.0',
                 'dec1.0', 'dec1.2.body.0'):  # fmt: skip
        keys += [f'{name}.weight', f'{name}.bias']
    for block in BLOCK_LIST:
        b = f'{block}.gated.0'
        keys += [f'{b}.norm.weight', f'{b}.fc1.weight', f'{b}.fc1.bias', f'{b}.fc2.weight', f'{b}.fc2.bias']
        if block != 'latent.1':
            keys += [f'{b}.conv.conv.weight', f'{b}.conv.conv.bias']
    return keys


class GateRArch(Architecture[GateR]):
    def __init__(self):
        super().__init__(uid='GateR', detect=KeyCondition.has_all(*_detect_keys()))

    def load(self, state: Mapping[str, object]) -> GateR:
        dim, in_ch = state['in_to_dim.weight'].shape[:2]
        num_blocks = [get_seq_len(state, block + '.gated') for block in BLOCK_LIST]
        latent_att = 'latent.1.gated.0.conv.conv.weight' not in state
        model = GateR(dim=dim, in_ch=in_ch, num_blocks=num_blocks, latent_att=latent_att)
        return self._enhance_model(model=model, in_channels=in_ch, out_channels=int(in_ch), upscale=1, name='GateR')
