"""Real-CUGAN loader (drop-in for ``resselt/archs/cugan/__init__.py``: same detection, same variant inference and metadata)."""

from __future__ import annotations

from typing import Literal, Mapping, Union

import torch

from ...factory import Architecture, KeyCondition
from .arch import UpCunet2x, UpCunet2x_fast, UpCunet3x, UpCunet4x

_CUGAN = Union[UpCunet2x, UpCunet3x, UpCunet4x, UpCunet2x_fast]


class CUGANArch(Architecture[_CUGAN]):
    def __init__(self):
        super().__init__(
            uid='CuGAN',
            detect=KeyCondition.has_all(
                'unet1.conv1.conv.0.weight',
                'unet1.conv1.conv.2.weight',
                'unet1.conv1_down.weight',
                'unet1.conv2.conv.0.weight',
                'unet1.conv2.conv.2.weight',
                'unet1.conv2.seblock.conv1.weight',
                'unet1.conv2_up.weight',
                'unet1.conv_bottom.weight',
                'unet2.conv1.conv.0.weight',
                'unet2.conv1_down.weight',
                'unet2.conv2.conv.0.weight',
                'unet2.conv2.seblock.conv1.weight',
                'unet2.conv3.conv.0.weight',
                'unet2.conv3.seblock.conv1.weight',
                'unet2.conv3_up.weight',
                'unet2.conv4.conv.0.weight',
                'unet2.conv4_up.weight',
                'unet2.conv5.weight',
                'unet2.conv_bottom.weight',
            ),
        )

    def load(self, state_dict: Mapping[str, object]) -> _CUGAN:
        scale: Literal[2, 3, 4]
        pro = False
        if 'pro' in state_dict:
            pro = True
            state_dict['pro'] = torch.zeros(1)  # as the reference: the buffer's value is not part of the checkpoint's meaning
        in_channels = state_dict['unet1.conv1.conv.0.weight'].shape[1]
        if 'conv_final.weight' in state_dict and in_channels == 12:
            scale, in_channels, out_channels = 2, 3, 3  # hard coded in UpCunet2x_fast
            model = UpCunet2x_fast(in_channels=in_channels, out_channels=out_channels)
        elif 'conv_final.weight' in state_dict:
            scale, out_channels = 4, 3  # hard coded in UpCunet4x
            model = UpCunet4x(in_channels=in_channels, out_channels=out_channels, pro=pro)
        elif state_dict['unet1.conv_bottom.weight'].shape[2] == 5:
            scale, out_channels = 3, state_dict['unet2.conv_bottom.weight'].shape[0]
            model = UpCunet3x(in_channels=in_channels, out_channels=out_channels, pro=pro)
        else:
            scale, out_channels = 2, state_dict['unet2.conv_bottom.weight'].shape[0]
            model = UpCunet2x(in_channels=in_channels, out_channels=out_channels, pro=pro)
        return self._enhance_model(model=model, in_channels=in_channels, out_channels=out_channels, upscale=scale, name='CUGAN')
