"""LAWFFT loader (drop-in for ``resselt/archs/lawfft/__init__.py``: the same 30 detection keys, the same inference and metadata).

One deliberate difference in how the module is built, none in what is inferred: the reference hands its module the float ratios it
inferred (``split = 1 / (dim / local)``, ``t_mid_factor``, ``mlp_factor``) and the module recomputes the widths with ``int(ratio * dim)``,
which lands on ``local - 1`` for some (dim, local) pairs (tests/golden/lawfft_probe.npz records one: its own module then rejects the state
dict).  Here ``local``, the FSAS width, ``to_hidden``'s rows and FeedForward's width are read from the checkpoint's shapes and handed over
beside the ratios.  An ``unshuffle_mod`` checkpoint that still carries ``in_to_dim.weight`` is inferred as the reference infers it and then
refused by the module.
"""

from __future__ import annotations

from typing import Mapping

from ...factory import Architecture, KeyCondition
from ...utilities.state_dict import get_seq_len
from .arch import LAWFFT, SAMPLE_MODS

_B = 'body.0.residual.0'
_T = f'{_B}.token_mix.1'
_C = f'{_B}.channel_mix1'
DETECTION_KEYS = (
    'in_to_dim.weight', 'in_to_dim.bias', f'{_B}.token_mix.0.weight', f'{_B}.token_mix.0.bias',
    f'{_T}.local.0.kernel_gen.1.weight', f'{_T}.local.0.kernel_gen.1.bias', f'{_T}.local.0.kernel_gen.3.weight', f'{_T}.local.0.kernel_gen.3.bias',
    f'{_T}.local.1.kernel_gen.1.weight', f'{_T}.local.1.kernel_gen.1.bias', f'{_T}.local.1.kernel_gen.3.weight', f'{_T}.local.1.kernel_gen.3.bias',
    f'{_T}.att.to_hidden.weight', f'{_T}.att.to_hidden.bias', f'{_T}.att.to_hidden_dw.weight', f'{_T}.att.to_hidden_dw.bias',
    f'{_T}.att.project_out.weight', f'{_T}.att.project_out.bias', f'{_T}.att.norm.weight', f'{_T}.att.norm.bias', f'{_T}.last.weight', f'{_T}.last.bias',
    f'{_C}.0.weight', f'{_C}.0.bias', f'{_C}.1.project_in.weight', f'{_C}.1.project_in.bias', f'{_C}.1.dwconv.weight', f'{_C}.1.dwconv.bias',
    f'{_C}.1.project_out.weight', f'{_C}.1.project_out.bias',
)  # fmt: skip


class LAWFFTArch(Architecture[LAWFFT]):
    def __init__(self):
        super().__init__(uid='LAWFFT', detect=KeyCondition.has_all(*DETECTION_KEYS))

    def load(self, state: Mapping[str, object]) -> LAWFFT:
        _, index, scale, dim, in_ch, mid_dim, _ = (int(v) for v in state['upscale.MetaUpsample'])
        unshuffle_mod = 'in_to_dim.1.weight' in state
        window_size = int(state['window_size'])
        local = int(state[f'{_T}.local.0.kernel_gen.1.bias'].shape[0])
        split = 1 / (dim / local)
        n_rblock = get_seq_len(state, 'body')
        n_mblock = get_seq_len(state, 'body.0.residual') - 1
        global_dim = dim - int(dim * split)  # (what the reference divides by: dim - local, or one more where the float product falls short)
        rows = int(state[f'{_T}.att.to_hidden.bias'].shape[0])
        fsas = int(state[f'{_T}.att.norm.weight'].shape[0])
        hidden = int(state[f'{_C}.1.project_out.weight'].shape[1])
        t_mid_factor = rows / global_dim / 3
        mlp_factor = int(state[f'{_C}.1.project_in.bias'].shape[0]) / dim / 2
        model = LAWFFT(in_ch=in_ch, dim=dim, split=split, scale=scale, n_rblock=n_rblock, n_mblock=n_mblock, t_mid_factor=t_mid_factor,
                       window_size=window_size, mlp_factor=mlp_factor, unshuffle_mod=unshuffle_mod, upsampler=SAMPLE_MODS[index], mid_dim=mid_dim,
                       local=local, fsas=fsas, hidden=hidden, to_hidden_rows=rows)  # fmt: skip
        return self._enhance_model(model=model, in_channels=in_ch, out_channels=in_ch, upscale=scale, name='LAWFFT')
