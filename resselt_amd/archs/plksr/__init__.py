"""PLKSR / RealPLKSR loader (drop-in for ``resselt/archs/plksr/__init__.py``: same detection, same inferred shapes and metadata)."""

from __future__ import annotations

from typing import Mapping, Union

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len, pixelshuffle_scale
from .arch import plksr, realplksr

_PLKSR = Union[plksr, realplksr]


class PLKSRArch(Architecture[_PLKSR]):
    def __init__(self):
        super().__init__(
            uid='PLKSR',
            detect=KeyCondition.has_all(
                'feats.0.weight',
                KeyCondition.has_any('feats.1.lk.conv.weight', 'feats.1.lk.convs.0.weight', 'feats.1.lk.mn_conv.weight'),
                'feats.1.refine.weight',
                KeyCondition.has_any('feats.1.channe_mixer.0.weight', 'feats.1.channel_mixer.0.weight'),
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> _PLKSR:
        kernel_size = 17
        in_nc = state_dict['feats.0.weight'].shape[1]
        dim = state_dict['feats.0.weight'].shape[0]
        total = get_seq_len(state_dict, 'feats')
        use_ea = 'feats.1.attn.f.0.weight' in state_dict
        scale = pixelshuffle_scale(state_dict[f'feats.{total - 1}.weight'].shape[0], in_nc)
        if 'feats.1.channe_mixer.0.weight' in state_dict:  # PLKSR (the reference's key has this spelling)
            name = 'PLKSR'
            k0 = state_dict['feats.1.channe_mixer.0.weight'].shape[2]
            k2 = state_dict['feats.1.channe_mixer.2.weight'].shape[2]
            ccm_type = {(3, 1): 'CCM', (3, 3): 'DCCM', (1, 3): 'ICCM'}.get((k0, k2))
            if ccm_type is None:
                raise ValueError('Unknown CCM type')
            if 'feats.1.lk.conv.weight' in state_dict:
                lk_type, lk = 'PLK', state_dict['feats.1.lk.conv.weight']
                kernel_size = lk.shape[2]
            elif 'feats.1.lk.convs.0.weight' in state_dict:
                lk_type, lk = 'SparsePLK', state_dict['feats.1.lk.convs.0.weight']
            else:
                lk_type, lk = 'RectSparsePLK', state_dict['feats.1.lk.mn_conv.weight']
                kernel_size = lk.shape[2]
            model = plksr(dim=dim, n_blocks=total - 2, upscaling_factor=scale, ccm_type=ccm_type, kernel_size=kernel_size,
                          split_ratio=lk.shape[0] / dim, lk_type=lk_type, use_ea=use_ea, in_ch=in_nc)  # fmt: skip
        else:  # RealPLKSR
            name = 'RealPLKSR'
            lk = state_dict['feats.1.lk.conv.weight']
            model = realplksr(dim=dim, n_blocks=total - 3, upscaling_factor=scale, kernel_size=lk.shape[2], split_ratio=lk.shape[0] / dim,
                              use_ea=use_ea, dysample='to_img.init_pos' in state_dict, in_ch=in_nc)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_nc, out_channels=in_nc, upscale=scale, name=name)
