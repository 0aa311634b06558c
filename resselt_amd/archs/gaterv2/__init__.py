"""GateRv2 loader (drop-in for ``resselt/archs/gaterv2/__init__.py``): the same detection keys, the same inference and metadata for x1
checkpoints.  Above x1 it departs from the reference on purpose:

* the reference's ``load`` reads ``state['to_img.MetaUpsample']`` where the state dict has ``upsample.MetaUpsample`` and raises ``KeyError``,
  so it loads x1 checkpoints only.  This loader reads ``upsample.MetaUpsample`` (scale, head and ``mid_dim``) and loads them;
* the reference module keeps ``self.scale = 1`` and crops the upscaled image to the input's size; the engine returns the full image and
  ``ModelMetadata.upscale`` is the scale.

No MetaUpsample buffer means x1 with a plain ``dim_to_in`` convolution.  Configurations the reference loads but the engine does not build
raise ``NotImplementedError`` from the constructor (archs/gaterv2/arch.py).
"""

from __future__ import annotations

from typing import Mapping

from ...engine.uniupsample import SAMPLE_MODS
from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import GateRV2

_MG = ('gamma0', 'gamma1', 'local.0.scale', 'local.0.offset', 'local.1.weight', 'local.1.bias', 'local.2.weight', 'local.2.bias', 'sca.1.weight',
       'sca.1.bias', 'glob.norm.scale', 'glob.norm.offset', 'glob.fc1.weight', 'glob.fc1.bias', 'glob.token_mix.dwconv_hw.weight',
       'glob.token_mix.dwconv_hw.bias', 'glob.token_mix.dwconv_w.weight', 'glob.token_mix.dwconv_w.bias', 'glob.token_mix.dwconv_h.weight',
       'glob.token_mix.dwconv_h.bias', 'glob.fc2.weight', 'glob.fc2.bias')  # fmt: skip
_LATENT = ('norm.scale', 'norm.offset', 'fc1.weight', 'fc1.bias', 'token_mix.query_conv.weight', 'token_mix.query_conv.bias', 'token_mix.key_conv.weight',
           'token_mix.key_conv.bias', 'token_mix.value_conv.weight', 'token_mix.value_conv.bias', 'fc2.weight', 'fc2.bias')  # fmt: skip


def detection_keys() -> tuple:
    """The reference's list: the first block of the first TWO encoder and decoder levels, the first latent block."""
    keys = ['in_to_dim.weight', 'in_to_dim.bias']
    for j in (0, 1):
        keys += [f'encode.{j}.gated.0.{k}' for k in _MG] + [f'encode.{j}.scale.0.weight']
    keys += [f'latent.0.{k}' for k in _LATENT]
    for j in (0, 1):
        keys += [f'decode.{j}.scale.0.weight'] + [f'decode.{j}.gated.0.{k}' for k in _MG] + [f'decode.{j}.shor.weight', f'decode.{j}.shor.bias']
    return tuple(keys)


DETECTION_KEYS = detection_keys()


class GateRV2Arch(Architecture[GateRV2]):
    def __init__(self):
        super().__init__(uid='GateRv2', detect=KeyCondition.has_all(*DETECTION_KEYS))

    @staticmethod
    def hyperparameters(state: Mapping[str, object]) -> dict:
        """What the reference's ``load`` infers, under its constructor's argument names (above x1: what it would infer from the buffer the
        state dict really has)."""
        dim, in_ch = (int(v) for v in state['in_to_dim.weight'].shape[:2])
        enc_blocks = [get_seq_len(state, f'encode.{i}.gated') for i in range(get_seq_len(state, 'encode'))]
        dec_blocks = [get_seq_len(state, f'decode.{i}.gated') for i in range(get_seq_len(state, 'decode'))]
        if 'upsample.MetaUpsample' in state:
            _, index, scale, _, _out_ch, upsample_dim, _ = (int(v) for v in state['upsample.MetaUpsample'])
            upsampler = SAMPLE_MODS[index]
        else:
            scale, upsample_dim, upsampler = 1, 32, 'conv'
        return dict(in_ch=in_ch, dim=dim, enc_blocks=enc_blocks, dec_blocks=dec_blocks, num_latent=get_seq_len(state, 'latent'), scale=scale,
                    upsample=upsampler, upsample_mid_dim=upsample_dim)  # fmt: skip

    def load(self, state: Mapping[str, object]) -> GateRV2:
        hp = self.hyperparameters(state)
        model = GateRV2(**hp)
        return self._enhance_model(model=model, in_channels=hp['in_ch'], out_channels=hp['in_ch'], upscale=hp['scale'], name='GateRv2')
