"""FIGSR loader (drop-in for ``resselt/archs/figsr/__init__.py``: the same 57 detection keys, the same inference and metadata; the
reference reports ``out_channels = in_nc``).

Two deliberate differences in how the module is built, none in what is inferred: ``hidden`` is read from the ``fc1`` shape and handed over
beside the ratio the reference infers (``fc1 rows / 2 / dim``), as GFISRv2's loader does; and the block counts of the two halves are
handed over as the checkpoint has them, so that a checkpoint whose halves are not the (n // 2, n - n // 2) split -- which the reference
module cannot take -- is refused by name.  A checkpoint with one block has an empty first half and is not detected, as in the reference.
"""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import FIGSR, SAMPLE_MODS3

_NORM = ('scale', 'offset', 'eps', 'rms')
_BLOCK = (
    *(f'norm.{k}' for k in _NORM), 'fc1.weight', 'fc1.bias', *(f'conv.fu.rn.{k}' for k in _NORM), *(f'conv.fu.post_norm.{k}' for k in _NORM),
    'conv.fu.fdc.weight', 'conv.fu.fdc.bias', 'conv.fu.fpe.weight', 'conv.fu.fpe.bias', 'conv.convhw.weight', 'conv.convhw.bias',
    'conv.convw.weight', 'conv.convw.bias', 'conv.convh.weight', 'conv.convh.bias', 'fc2.weight', 'fc2.bias',
)  # fmt: skip
DETECTION_KEYS = (
    'in_to_dim.weight', 'in_to_dim.bias', *(f'gfisr_body_half.0.{k}' for k in _BLOCK), *(f'gfisr_body_half_2.0.{k}' for k in _BLOCK),
    'cat_to_dim.weight', 'cat_to_dim.bias', 'upscale.MetaUpsample',
)  # fmt: skip
_B = 'gfisr_body_half.0'


class FIGSRArch(Architecture[FIGSR]):
    def __init__(self):
        super().__init__(uid='FIGSR', detect=KeyCondition.has_all(*DETECTION_KEYS))

    def load(self, state: Mapping[str, object]) -> FIGSR:
        _, index, scale, _, out_nc, mid_dim, _ = (int(v) for v in state['upscale.MetaUpsample'])
        dim, in_nc = (int(v) for v in state['in_to_dim.weight'].shape[:2])
        hidden = int(state[f'{_B}.fc1.weight'].shape[0]) // 2
        expansion_ratio = int(state[f'{_B}.fc1.weight'].shape[0]) / 2 / dim
        halves = (get_seq_len(state, 'gfisr_body_half'), get_seq_len(state, 'gfisr_body_half_2') - 1)
        gc = int(state[f'{_B}.conv.convh.bias'].shape[0])
        square_kernel_size = int(state[f'{_B}.conv.convhw.weight'].shape[2])
        band_kernel_size = int(state[f'{_B}.conv.convh.weight'].shape[2])
        model = FIGSR(in_nc=in_nc, dim=dim, expansion_ratio=expansion_ratio, scale=scale, out_nc=out_nc, upsampler=SAMPLE_MODS3[index],
                      mid_dim=mid_dim, n_blocks=sum(halves), gc=gc, square_kernel_size=square_kernel_size, band_kernel_size=band_kernel_size,
                      hidden=hidden, halves=halves)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_nc, out_channels=in_nc, upscale=scale, name='FIGSR')
