"""MoESR on the MI355X engine (reference module: ``resselt/archs/moesr/arch.py:190-227``), eval-mode semantics.

The gated block is MoSRv2's (``archs/mosrv2/arch.py``, shared through ``_GatedBase``): channel LayerNorm, fc1, the Mish gate over the
Inception depthwise step (one rsa_gated_dwconv launch), fc2 + Mish, ``x * gamma + shortcut``.  What MoESR adds is the topology around the
blocks, and rsa_moesr_stream (csrc/moesr.hip) carries it: every ``Blocks`` group ends in an MSG stage -- conv dim -> dim/4,
PixelUnshuffle(2), LeakyReLU 0.1, three gated blocks at half resolution, conv dim -> 4 dim, PixelShuffle(2), LeakyReLU 0.1, ``+ x`` -- so the
f32 residual stream changes resolution twice per group.  One launch of that kernel closes a step of the stream and opens the next one:

  mode 0  block tail: fc2 + Mish (f32 map) * gamma + stream -> stream, and the next block's LayerNorm as planes
  mode 1  MSG entry: the down-convolution's f32 map (LeakyReLU in its epilogue) -> the half-resolution stream + LayerNorm planes
  mode 2  MSG exit: the up-convolution's f32 map -> depth-to-space + stream (+ the trunk residual after the last group)

A block whose successor is a convolution (the group's last block feeds MSG.down, the MSG's last block feeds MSG.up, the last group feeds the
head) gets plain planes instead of LayerNorm planes, and the MSG's last block writes no stream at all.  Only the very first block's norm is
an rsa_layernorm launch (of in_to_dim's output).

Front end: ``check_img_size``'s reflect pad to a multiple of 2, fused into rsa_nchw_to_planes.  Head: the five UniUpsample modes of
``engine/uniupsample.py``; the output is cropped by ``Plan.output``.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import lib_moesr as LM
from ...engine import ops
from ...engine.base import Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16
from ...engine.uniupsample import SAMPLE_MODS, Head
from ..mosr.arch import LN_EPS, _check_dims, _conv_weights, _GatedBase

MAX_DIM = 128  # rsa_moesr_stream keeps a pixel's channels in registers
MSG_BLOCKS = 3
LRELU = 0.1


class MoESR(_GatedBase):
    def __init__(self, in_ch: int = 3, out_ch: int = 3, scale: int = 4, dim: int = 64, n_blocks: int = 9, n_block: int = 4, expansion_factor: float = 8 / 3,
                 expansion_msg: float = 1.5, upsampler: str = 'pixelshuffledirect', upsample_dim: int = 64, hidden: int | None = None,
                 hidden_msg: int | None = None) -> None:  # fmt: skip
        """``hidden`` / ``hidden_msg``: the widths of fc2's input in the groups' blocks and in the MSG's blocks, where a checkpoint gives them
        (the loader reads them from the ``fc1`` shapes); otherwise ``int(ratio * dim)`` as the reference computes them."""
        super().__init__()
        if dim % 8:
            raise NotImplementedError(f'MoESR: dim must be a multiple of 8 (got {dim})')
        if dim > MAX_DIM:
            raise NotImplementedError(f'MoESR: dim above {MAX_DIM} is not built (got {dim}; rsa_moesr_stream keeps a pixel\'s channels in registers)')
        _check_dims('MoESR', dim, in_ch)
        if n_blocks < 1 or n_block < 1:
            raise NotImplementedError('MoESR: at least one group of at least one block')
        if upsampler not in SAMPLE_MODS:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')
        if upsampler == 'conv':
            scale = 1
        hidden = int(expansion_factor * dim) if hidden is None else int(hidden)
        hidden_msg = int(expansion_msg * dim) if hidden_msg is None else int(hidden_msg)
        if hidden < dim or hidden_msg < dim:
            raise NotImplementedError(f'MoESR: hidden must be at least dim (got {hidden} and {hidden_msg} in the MSG for dim {dim})')
        self.in_ch, self.out_ch, self.scale, self.dim, self.n_blocks, self.n_block = in_ch, out_ch, scale, dim, n_blocks, n_block
        self.expansion_factor, self.expansion_msg, self.hidden, self.hidden_msg = expansion_factor, expansion_msg, hidden, hidden_msg
        self.head, self.upsample_dim, self.gc = upsampler, upsample_dim, int(dim * 0.125)
        self._gate_hidden = hidden
        # (UniUpsample of this family gives DySample the features themselves: no mid_dim convolution in front of it)
        self.mid_dim = dim if upsampler == 'dysample' else upsample_dim
        self.up = Head('upscale', upsampler, scale, dim, out_ch, self.mid_dim, version=1, meta_mid_dim=upsample_dim)
        shapes: dict = {'in_to_dim.weight': (dim, in_ch, 3, 3), 'in_to_dim.bias': (dim,)}
        for g in range(n_blocks):
            for j in range(n_block):
                self._block_shapes(shapes, f'blocks.{g}.blocks.{j}', hidden)
            m = f'blocks.{g}.msg'
            shapes[f'{m}.down.0.weight'], shapes[f'{m}.down.0.bias'] = (dim // 4, dim, 3, 3), (dim // 4,)
            for j in range(MSG_BLOCKS):
                self._block_shapes(shapes, f'{m}.gated.{j}', hidden_msg)
            shapes[f'{m}.up.0.weight'], shapes[f'{m}.up.0.bias'] = (4 * dim, dim, 3, 3), (4 * dim,)
        buffers: dict = {}
        self.up.shapes(shapes, buffers, whole_planes='MoESR')
        build_param_tree(self, shapes, buffers)

    def _block_shapes(self, shapes: dict, b: str, hidden: int) -> None:
        dim, gc = self.dim, self.gc
        shapes[f'{b}.gamma'] = (1, dim, 1, 1)
        shapes[f'{b}.norm.weight'] = (dim,)
        shapes[f'{b}.norm.bias'] = (dim,)
        shapes[f'{b}.fc1.weight'] = (2 * hidden, dim, 3, 3)
        shapes[f'{b}.fc1.bias'] = (2 * hidden,)
        for name, (kh, kw) in (('dwconv_hw', (3, 3)), ('dwconv_w', (1, 11)), ('dwconv_h', (11, 1))):
            shapes[f'{b}.conv.{name}.weight'] = (gc, 1, kh, kw)
            shapes[f'{b}.conv.{name}.bias'] = (gc,)
        shapes[f'{b}.fc2.weight'] = (dim, hidden, 3, 3)
        shapes[f'{b}.fc2.bias'] = (dim,)

    # ---- the hooks of _GatedBase; ``_gate_hidden`` is the width of the blocks being packed / emitted (the groups' or the MSG's)
    def _gate_groups(self):
        gc, h, d = self.gc, self._gate_hidden, self.dim
        return [(h - d, (1, 1)), (d - 3 * gc, (1, 1)), (gc, (3, 3)), (gc, (1, 11)), (gc, (11, 1))]

    def _dw_weights(self, sd, b, s):
        name = ('dwconv_hw', 'dwconv_w', 'dwconv_h')[s]
        return sd[f'{b}.conv.{name}.weight'], sd[f'{b}.conv.{name}.bias']

    def _block_gamma(self, sd, b):
        return sd[f'{b}.gamma'].reshape(-1).contiguous()

    def _of_width(self, hidden: int, fn, *args):
        self._gate_hidden = hidden
        try:
            return fn(*args)
        finally:
            self._gate_hidden = self.hidden

    def _group_blocks(self, g: int):
        """(key prefix, hidden) of the group's blocks, then of its MSG's."""
        return ([(f'blocks.{g}.blocks.{j}', self.hidden) for j in range(self.n_block)],
                [(f'blocks.{g}.msg.gated.{j}', self.hidden_msg) for j in range(MSG_BLOCKS)])  # fmt: skip

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
        W: dict = {'conv0': cw(sd['in_to_dim.weight'], sd['in_to_dim.bias'])}
        for g in range(self.n_blocks):
            full, half = self._group_blocks(g)
            for b, hidden in full + half:
                self._of_width(hidden, self._pack_block, W, sd, b, products, device)
            for name in ('down', 'up'):
                W[f'blocks.{g}.msg.{name}'] = cw(sd[f'blocks.{g}.msg.{name}.0.weight'], sd[f'blocks.{g}.msg.{name}.0.bias'])
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        d = self.dim
        blk = lambda h: 9 * d * 2 * h + (9 + 22) * self.gc + 9 * h * d  # noqa: E731
        msg = 9 * d * (d // 4) + (MSG_BLOCKS * blk(self.hidden_msg) + 9 * d * 4 * d) // 4  # the stage between the two convolutions runs on a quarter of the pixels
        head = self.up.macs()
        if self.up.dys_index is not None:
            head += d * 8 * self.scale * self.scale * 2
        return 9 * self.in_ch * d + self.n_blocks * (self.n_block * blk(self.hidden) + msg) + head

    def _stream(self, plan: Plan, mode: int, n, H, Wd, a, *, gamma=None, s_in=None, s2_in=None, s_out=None, norm=None, planes=None):
        """One rsa_moesr_stream launch; H x Wd is the output stream.  ``norm``: (weight, bias) of the LayerNorm the planes hold, None = plain."""
        sp = LM.MoesrStreamParams()
        sp.batch, sp.H, sp.W, sp.C, sp.mode = n, H, Wd, self.dim, mode
        sp.a_H, sp.a_W = ((H, Wd), (2 * H, 2 * Wd), (H // 2, Wd // 2))[mode]
        sp.a = a.data_ptr()
        for key, t in (('gamma', gamma), ('s_in', s_in), ('s2_in', s2_in), ('s_out', s_out)):
            setattr(sp, key, None if t is None else t.data_ptr())
        if planes is not None:
            planes.bind(sp, 'out')
            sp.fmt = planes.fmt
            if norm is not None:
                sp.ln_gamma, sp.ln_beta, sp.eps = norm[0].data_ptr(), norm[1].data_ptr(), LN_EPS
        # byte model (csrc/moesr.hip): a, s_in, s2_in read once, the stream and the planes written once
        maps = 1 + sum(t is not None for t in (s_in, s2_in, s_out))
        halves = 0 if planes is None else 2 if planes.lo is not None else 1
        form = 'no planes' if planes is None else 'LayerNorm planes' if norm is not None else 'plain planes'
        label = f'mode {mode}, {form}, {"stream" if s_out is not None else "no stream"}{", + trunk" if s2_in is not None else ""}, {H}x{Wd}'
        plan.launch('rsa_moesr_stream', sp, meta=dict(kernel='rsa_moesr_stream', flop=0, bytes=n * H * Wd * self.dim * (4 * maps + 2 * halves), label=label))

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        s, dim = self.scale, self.dim
        H, Wd = h0 + h0 % 2, w0 + w0 % 2
        if H - h0 >= h0 or Wd - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to a multiple of 2')
        Hh, Wh = H // 2, Wd // 2
        pd = dim // 8
        with_lo = products == 3
        x_pl = plan.planes(n, 1, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)  # check_img_size's reflect pad, fused

        trunk, S, R = (plan.f32map(n, dim, H, Wd) for _ in range(3))  # in_to_dim's output (the trunk residual), the stream, fc2 + Mish
        Sh, Rh = plan.f32map(n, dim, Hh, Wh), plan.f32map(n, dim, Hh, Wh)
        D = plan.f32map(n, dim // 4, H, Wd)
        U = plan.f32map(n, 4 * dim, Hh, Wh)
        P, Ph = plan.planes(n, pd, H, Wd, with_lo), plan.planes(n, pd, Hh, Wh, with_lo)  # plain planes: what MSG.down / the head and MSG.up read
        bufs = self._of_width(self.hidden, self._block_buffers, plan, n, H, Wd, with_lo)
        bufs_h = self._of_width(self.hidden_msg, self._block_buffers, plan, n, Hh, Wh, with_lo)
        fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None

        plan.conv(ops.conv_params(W['conv0'], x_pl, H, Wd, out_f32=trunk))
        for g in range(self.n_blocks):
            full, half = self._group_blocks(g)
            last_group = g == self.n_blocks - 1
            for j, (b, hidden) in enumerate(full):
                first = g == 0 and j == 0  # the only block whose input is not normalised yet; its stream is the trunk residual, kept intact
                m = self._of_width(hidden, self._emit_block, plan, W[b], n, H, Wd, trunk if first else None, bufs)
                plan.conv(ops.conv_params(W[b]['fc2'], m, H, Wd, act=L.ACT_MISH, out_f32=R))
                nxt = W[full[j + 1][0]]['norm'] if j + 1 < len(full) else None
                self._stream(plan, 0, n, H, Wd, R, gamma=W[b]['gamma'], s_in=trunk if first else S, s_out=S, norm=nxt,
                             planes=bufs['norm'] if nxt else P)  # fmt: skip
            plan.conv(ops.conv_params(W[f'blocks.{g}.msg.down'], P, H, Wd, act=L.ACT_LRELU, act_param=LRELU, out_f32=D))
            self._stream(plan, 1, n, Hh, Wh, D, s_out=Sh, norm=W[half[0][0]]['norm'], planes=bufs_h['norm'])
            for j, (b, hidden) in enumerate(half):
                m = self._of_width(hidden, self._emit_block, plan, W[b], n, Hh, Wh, None, bufs_h)
                plan.conv(ops.conv_params(W[b]['fc2'], m, Hh, Wh, act=L.ACT_MISH, out_f32=Rh))
                nxt = W[half[j + 1][0]]['norm'] if j + 1 < len(half) else None  # the last one feeds MSG.up alone: plain planes, no stream
                self._stream(plan, 0, n, Hh, Wh, Rh, gamma=W[b]['gamma'], s_in=Sh, s_out=Sh if nxt else None, norm=nxt,
                             planes=bufs_h['norm'] if nxt else Ph)  # fmt: skip
            plan.conv(ops.conv_params(W[f'blocks.{g}.msg.up'], Ph, Hh, Wh, act=L.ACT_LRELU, act_param=LRELU, out_f32=U))
            if last_group:  # + the trunk residual; the head reads plain planes (and DySample the f32 features)
                self._stream(plan, 2, n, H, Wd, U, s_in=S, s2_in=trunk, s_out=fe32, planes=P)
            else:
                self._stream(plan, 2, n, H, Wd, U, s_in=S, s_out=S, norm=W[f'blocks.{g + 1}.blocks.0']['norm'], planes=bufs['norm'])
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        self.up.emit(plan, W, P, fe32, y, with_lo)
        return set_input
