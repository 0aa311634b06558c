"""EIMN loader (drop-in for ``resselt/archs/eimn/__init__.py``: the same detection keys, inferred hyper-parameters and metadata)."""

from __future__ import annotations

import re
from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len, pixelshuffle_scale
from .arch import EIMN

_BLOCK = re.compile(r'block(\d+)')


class EIMNArch(Architecture[EIMN]):
    def __init__(self):
        b = 'block1.0'
        convs = ('attn.region', 'attn.spatial_1', 'attn.spatial_2', 'attn.fusion', 'attn.proj_value.0', 'attn.proj_query.0', 'attn.out', 'mlp.linear_in',
                 'mlp.SAL', 'mlp.linear_out', 'mlp.DFFM.norm', 'mlp.DFFM.global_reduce', 'mlp.DFFM.local_reduce', 'mlp.DFFM.channel_expand',
                 'mlp.DFFM.spatial_expand')  # fmt: skip
        bn = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')
        super().__init__(
            uid='eimn',
            detect=KeyCondition.has_all(
                'head.0.weight', 'head.0.bias', 'tail.0.weight', 'tail.0.bias', f'{b}.layer_scale_1', f'{b}.layer_scale_2',
                *(f'{b}.norm1.{k}' for k in bn), *(f'{b}.norm2.{k}' for k in bn),
                *(f'{b}.{name}.{k}' for name in convs for k in ('weight', 'bias')),
                'norm1.weight', 'norm1.bias',
            ),
        )  # fmt: skip

    def load(self, state_dict: Mapping[str, object]) -> EIMN:
        num_stages = max(int(m.group(1)) for m in map(_BLOCK.search, state_dict.keys()) if m)
        depths = get_seq_len(state_dict, 'block1')
        # the hidden width straight from the checkpoint: through the reference's float mlp_ratio, int(dim * ratio) can land one lower
        hidden = state_dict['block1.0.mlp.linear_in.weight'].shape[0] // 2
        embed_dim = state_dict['head.0.weight'].shape[0]
        scale = pixelshuffle_scale(state_dict['tail.0.weight'].shape[0], 3)
        model = EIMN(embed_dims=embed_dim, scale=scale, depths=depths, hidden=hidden, num_stages=num_stages)
        return self._enhance_model(model=model, in_channels=3, out_channels=3, upscale=scale, name='EIMN')
