"""GateRV3 loader (drop-in for ``resselt/archs/gaterv3/__init__.py``): the same detection keys, the same inference and metadata, quirks
included:

* detection needs ``span_n_b.0.*``, so a checkpoint with ``span_blocks = 0`` is never detected and raises ``ArchitectureNotFound``;
* ``scale``, the head and ``mid_dim`` come from ``dim_to_in.MetaUpsample``; a dysample head without ``dim_to_in.0.weight`` has no front
  convolution and ``mid_dim = dim`` whatever the buffer records, and ``end_kernel`` is read from the shape of ``end_conv.weight``;
* no MetaUpsample buffer means x1 with a plain ``dim_to_in`` convolution; a missing ``gamma`` means ones (the module's own).

Configurations the reference loads but the engine does not build raise ``NotImplementedError`` from the constructor (archs/gaterv3/arch.py).
"""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import GateRV3

_MG = ('gamma0', 'gamma1', 'local.0.scale', 'local.0.offset', 'local.1.weight', 'local.1.bias', 'local.2.weight', 'local.2.bias', 'sca.1.weight',
       'sca.1.bias', 'glob.norm.scale', 'glob.norm.offset', 'glob.fc1.weight', 'glob.fc1.bias', 'glob.token_mix.dwconv_hw.weight',
       'glob.token_mix.dwconv_hw.bias', 'glob.token_mix.dwconv_w.weight', 'glob.token_mix.dwconv_w.bias', 'glob.token_mix.dwconv_h.weight',
       'glob.token_mix.dwconv_h.bias', 'glob.fc2.weight', 'glob.fc2.bias')  # fmt: skip
_C3 = ('sk.weight', 'conv.0.weight', 'conv.1.weight', 'conv.2.weight', 'eval_conv.weight')
SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')


def detection_keys() -> tuple:
    keys = ['in_to_dim.weight', 'in_to_dim.bias']
    keys += [f'gater_encode.0.gated.0.{k}' for k in _MG] + ['gater_encode.0.scale.0.weight']
    for spab in ('span_block0', 'span_n_b.0', 'span_end'):
        keys += [f'{spab}.{r}.{k}' for r in ('c1_r', 'c2_r', 'c3_r') for k in _C3]
    for sub in ('sk', 'conv.0', 'conv.1', 'conv.2', 'eval_conv'):
        keys += [f'sisr_end_conv.{sub}.weight', f'sisr_end_conv.{sub}.bias']
    keys += ['sisr_cat_conv.weight', 'sisr_cat_conv.bias', 'decode.0.scale.0.weight']
    keys += [f'decode.0.gated.0.{k}' for k in _MG] + ['decode.0.shor.weight', 'decode.0.shor.bias']
    return tuple(keys)


DETECTION_KEYS = detection_keys()


class GateRV3Arch(Architecture[GateRV3]):
    def __init__(self):
        super().__init__(uid='GateRV3', detect=KeyCondition.has_all(*DETECTION_KEYS))

    @staticmethod
    def hyperparameters(state: Mapping[str, object]) -> dict:
        """What the reference's ``load`` infers, under its constructor's argument names."""
        dim, in_ch = (int(v) for v in state['in_to_dim.weight'].shape[:2])
        enc_blocks = [get_seq_len(state, f'gater_encode.{i}.gated') for i in range(get_seq_len(state, 'gater_encode'))]
        dec_blocks = [get_seq_len(state, f'decode.{i}.gated') for i in range(get_seq_len(state, 'decode'))]
        end_kernel = 1
        if 'dim_to_in.MetaUpsample' in state:
            _, index, scale, _, _out_ch, upsample_dim, _ = (int(v) for v in state['dim_to_in.MetaUpsample'])
            upsampler = SAMPLE_MODS[index]
            if upsampler == 'dysample' and 'dim_to_in.0.weight' not in state:
                upsample_dim = dim
                end_kernel = int(state['dim_to_in.0.end_conv.weight'].shape[2])
            elif upsampler == 'dysample':
                end_kernel = int(state['dim_to_in.2.end_conv.weight'].shape[2])
        else:
            scale, upsample_dim, upsampler = 1, 32, 'conv'
        return dict(in_ch=in_ch, dim=dim, enc_blocks=enc_blocks, dec_blocks=dec_blocks, num_latent=get_seq_len(state, 'latent'), scale=scale,
                    upsample=upsampler, upsample_mid_dim=upsample_dim, attention='latent.0.token_mix.qkv_dwconv.weight' in state,
                    span_blocks=get_seq_len(state, 'span_n_b'), end_kernel=end_kernel)  # fmt: skip

    def load(self, state: Mapping[str, object]) -> GateRV3:
        hp = self.hyperparameters(state)
        model = GateRV3(**hp)
        return self._enhance_model(model=model, in_channels=hp['in_ch'], out_channels=hp['in_ch'], upscale=hp['scale'], name='GateRV3')
