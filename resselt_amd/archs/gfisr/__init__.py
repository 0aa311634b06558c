"""GFISR (v1) loader (drop-in for ``resselt/archs/gfisr/__init__.py``, whose class is misnamed ``GateRV3Arch``; its uid is ``GFISR``): the
same 16 detection keys, the same inference and metadata, quirks included:

* the reference hands ``upsample_dim=`` to a constructor whose parameter is ``mid_dim``, so the value lands in ``**kwargs`` and the module
  is always built with ``mid_dim = 32``: a checkpoint whose head has another ``mid_dim`` fails in the strict ``load_state_dict`` with a
  size mismatch, here as there;
* detection needs ``in_to_dim.weight``, so a ``pixel_unshuffle`` checkpoint (``in_to_dim.1.weight``) is never detected and raises
  ``ArchitectureNotFound``, although ``load()`` has a branch for it (kept, as the reference keeps it).  Such a model can be built directly.

One deliberate difference in how the module is built, none in what is inferred: ``hidden`` is read from the ``fc1`` shape and handed over
beside the expansion ratio, as GFISRv2's loader does.
"""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import FIXED_MID_DIM, GFISR, SAMPLE_MODS3

_B = 'net.0'
DETECTION_KEYS = (
    'in_to_dim.weight', 'in_to_dim.bias', f'{_B}.gamma', f'{_B}.norm.weight', f'{_B}.norm.bias', f'{_B}.fc1.weight', f'{_B}.fc1.bias',
    f'{_B}.conv.dwconv_hw.weight', f'{_B}.conv.dwconv_hw.bias', f'{_B}.conv.dwconv_w.weight', f'{_B}.conv.dwconv_w.bias',
    f'{_B}.conv.dwconv_h.weight', f'{_B}.conv.dwconv_h.bias', f'{_B}.fc2.weight', f'{_B}.fc2.bias', 'dim_to_out.MetaUpsample',
)  # fmt: skip


class GFISRArch(Architecture[GFISR]):
    def __init__(self):
        super().__init__(uid='GFISR', detect=KeyCondition.has_all(*DETECTION_KEYS))

    def load(self, state: Mapping[str, object]) -> GFISR:
        _, index, scale, _, out_ch, _upsample_dim, _ = (int(v) for v in state['dim_to_out.MetaUpsample'])
        fft_mode = f'{_B}.conv.fsas.ln.weight' in state
        if 'in_to_dim.weight' in state:
            dim, in_nc = (int(v) for v in state['in_to_dim.weight'].shape[:2])
            pixel_unshuffle = False
        else:
            dim, in_nc = (int(v) for v in state['in_to_dim.1.weight'].shape[:2])
            in_nc = in_nc // 16 if in_nc % 16 == 0 else in_nc // 4
            pixel_unshuffle = True
        n_blocks = get_seq_len(state, 'net')
        hidden = int(state[f'{_B}.fc1.bias'].shape[0]) // 2
        expansion_ratio = state[f'{_B}.fc1.bias'].shape[0] / 2 / dim
        model = GFISR(in_nc=in_nc, dim=dim, expansion_ratio=expansion_ratio, fft_mode=fft_mode, scale=scale, out_nc=out_ch,
                      upsampler=SAMPLE_MODS3[index], mid_dim=FIXED_MID_DIM, pixel_unshuffle=pixel_unshuffle, n_blocks=n_blocks, hidden=hidden)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_nc, out_channels=out_ch, upscale=scale, name='GFISR')
