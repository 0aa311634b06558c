"""MoSRv2 on the MI355X engine (reference module: ``resselt/archs/mosrv2/arch.py:281-337``), eval-mode semantics.

The gated block is MoSR's (``archs/mosr/arch.py``) with an InceptionDWConv2d (:174-210) as its depthwise step: cat(i, x_id) pass through,
x_hw / x_w / x_h go through 3x3, 1x11 and 11x1 depthwise convolutions -- one rsa_gated_dwconv launch with three segments.  The residual
``x * gamma + shortcut`` is rsa_group_norm_apply with statistics (0, 1), gain gamma and no shift: fc2 + Mish writes an f32 map, the apply
adds the stream and writes the next stream (and, after the last block, the trunk's input planes).  RMSNorm or LayerNorm as the checkpoint
says.

Front end: ``check_img_size``'s reflect pad and, with ``unshuffle_mod`` below x3, the PixelUnshuffle, fused into rsa_nchw_to_planes.
Heads (UniUpsample, :91-172): conv, pixelshuffledirect (final store through depth-to-space), pixelshuffle (LeakyReLU 0.01, shuffling stores
re-laid out as planes), nearest+conv (x2^n: the convolution's nearest-upsample-on-read; x3: the convolution before the upsampling is stored
with every output channel repeated 9 times through depth-to-space, which IS the nearest x3 map) and dysample (the shared DySample head after
the optional mid_dim conv + LeakyReLU 0.01).  ``self.short`` -- bilinear upsampling of the padded input -- is rsa_bilinear_add on the output.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import ops, plk
from ...engine.base import Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16
from ...engine.uniupsample import SAMPLE_MODS, Head, OwnMetaUpsample  # noqa: F401  (SAMPLE_MODS: re-exported)
from ..mosr.arch import _check_dims, _conv_weights, _GatedBase


class MoSRv2(OwnMetaUpsample, _GatedBase):  # (the reference's load_state_dict override: arch.py:319-321)
    def __init__(self, in_ch: int = 3, scale: int = 4, n_block: int = 24, dim: int = 64, upsampler: str = 'pixelshuffledirect', expansion_ratio: float = 1.5,
                 mid_dim: int = 32, unshuffle_mod: bool = True, rms_norm: bool = False) -> None:  # fmt: skip
        super().__init__()
        _check_dims('MoSRv2', dim, in_ch)
        if n_block < 1:
            raise NotImplementedError('MoSRv2: at least one block')
        self.scale, self.in_ch, self.n_block, self.dim, self.head, self.mid_dim, self.rms_norm = scale, in_ch, n_block, dim, upsampler, mid_dim, rms_norm
        self.unshuffle, self.s_int = 1, scale
        if unshuffle_mod and scale < 3:
            self.unshuffle, self.s_int = 4 // scale, 4
        hidden = int(expansion_ratio * dim)
        self.hidden, self.gc = hidden, int(dim * 0.125)
        if hidden < dim:
            raise NotImplementedError(f'MoSRv2: hidden = int(expansion_ratio * dim) must be at least dim (got {hidden})')
        self.up = Head('to_img', upsampler, self.s_int, dim, in_ch, mid_dim)
        self.first = 2 if self.unshuffle > 1 else 1
        u = self.unshuffle
        shapes: dict = {f'gblocks.{self.first - 1}.weight': (dim, in_ch * u * u, 3, 3), f'gblocks.{self.first - 1}.bias': (dim,)}
        for i in range(self.first, self.first + n_block):
            b = f'gblocks.{i}'
            if rms_norm:
                shapes[f'{b}.norm.scale'] = (dim, 1, 1)
                shapes[f'{b}.norm.offset'] = (dim, 1, 1)
            else:
                shapes[f'{b}.norm.weight'] = (dim,)
                shapes[f'{b}.norm.bias'] = (dim,)
            shapes[f'{b}.fc1.weight'] = (2 * hidden, dim, 3, 3)
            shapes[f'{b}.fc1.bias'] = (2 * hidden,)
            for name, (kh, kw) in (('dwconv_hw', (3, 3)), ('dwconv_w', (1, 11)), ('dwconv_h', (11, 1))):
                shapes[f'{b}.conv.{name}.weight'] = (self.gc, 1, kh, kw)
                shapes[f'{b}.conv.{name}.bias'] = (self.gc,)
            shapes[f'{b}.fc2.weight'] = (dim, hidden, 3, 3)
            shapes[f'{b}.fc2.bias'] = (dim,)
            shapes[f'{b}.gamma'] = (1, dim, 1, 1)
        t = self.first + n_block
        for k, (co, ci, ks) in ((t, (2 * dim, dim, 3)), (t + 2, (dim, 2 * dim, 3)), (t + 4, (dim, dim, 1))):
            shapes[f'gblocks.{k}.weight'] = (co, ci, ks, ks)
            shapes[f'gblocks.{k}.bias'] = (co,)
        buffers: dict = {}
        self.up.shapes(shapes, buffers, whole_planes='MoSRv2')
        build_param_tree(self, shapes, buffers)

    def _gate_groups(self):
        gc, h, d = self.gc, self.hidden, self.dim
        return [(h - d, (1, 1)), (d - 3 * gc, (1, 1)), (gc, (3, 3)), (gc, (1, 11)), (gc, (11, 1))]

    def _dw_weights(self, sd, b, s):
        name = ('dwconv_hw', 'dwconv_w', 'dwconv_h')[s]
        return sd[f'{b}.conv.{name}.weight'], sd[f'{b}.conv.{name}.bias']

    def _block_gamma(self, sd, b):
        return sd[f'{b}.gamma'].reshape(-1).contiguous()

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        dim = self.dim
        cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
        k0 = f'gblocks.{self.first - 1}'
        W: dict = {'conv0': cw(sd[f'{k0}.weight'], sd[f'{k0}.bias'])}
        for i in range(self.first, self.first + self.n_block):
            self._pack_block(W, sd, f'gblocks.{i}', products, device)
        last = self._trunk_tail(W, sd, self.first, products, device)
        W['tail2'] = cw(sd[f'gblocks.{last}.weight'], sd[f'gblocks.{last}.bias'])
        W['zeros'] = torch.zeros(dim, dtype=torch.float32, device=device)
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        d, h, u = self.dim, self.hidden, self.unshuffle
        blk = 9 * d * 2 * h + (9 + 22) * self.gc + 9 * h * d
        total = 9 * self.in_ch * u * u * d + self.n_block * blk + 9 * d * 2 * d * 2 + d * d + self.up.macs()
        return total // (u * u)

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        u, s, dim = self.unshuffle, self.s_int, self.dim
        Hp, Wp = h0 + (u - h0 % u) % u, w0 + (u - w0 % u) % u
        if Hp - h0 >= h0 or Wp - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to the unshuffle factor')
        H, Wd = Hp // u, Wp // u
        pd = dim // 8
        with_lo = products == 3
        dev = plan.device
        x_pl = plan.planes(n, (self.in_ch * u * u + 7) // 8, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl, unshuffle=u)  # check_img_size's reflect pad and the PixelUnshuffle, fused

        cur, nxt = plan.f32map(n, dim, H, Wd), plan.f32map(n, dim, H, Wd)
        R = plan.f32map(n, dim, H, Wd)
        feat = plan.planes(n, pd, H, Wd, with_lo)
        bufs = self._block_buffers(plan, n, H, Wd, with_lo)
        stats = self._unit_stats(n, dev)
        plan.keep.append(stats)
        plan.conv(ops.conv_params(W['conv0'], x_pl, H, Wd, out_f32=cur))
        for i in range(self.first, self.first + self.n_block):
            blk = W[f'gblocks.{i}']
            m = self._emit_block(plan, blk, n, H, Wd, cur, bufs)
            last = i == self.first + self.n_block - 1
            plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, act=L.ACT_MISH, out_f32=R))
            ap = plk.group_norm_apply_params(R, dim, 1, stats, blk['gamma'], W['zeros'], cur, feat if last else None, None if last else nxt)
            plan.launch('rsa_group_norm_apply', ap)
            cur, nxt = nxt, cur
        t1 = plan.planes(n, 2 * pd, H, Wd, with_lo)
        t2 = plan.planes(n, pd, H, Wd, with_lo)
        fe = plan.planes(n, pd, H, Wd, with_lo)
        plan.conv(ops.conv_params(W['tail0'], feat, H, Wd, act=L.ACT_MISH, out=t1))
        plan.conv(ops.conv_params(W['tail1'], t1, H, Wd, act=L.ACT_MISH, out=t2))
        fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None
        plan.conv(ops.conv_params(W['tail2'], t2, H, Wd, out=fe, out_f32=fe32))

        y = plan.output((n, self.in_ch, H * s, Wd * s), dtype, crop=(h0 * self.scale, w0 * self.scale))
        self.up.emit(plan, W, fe, fe32, y, with_lo)
        bp = L.BilinearAddParams()
        bp.batch, bp.C, bp.h, bp.w, bp.pad_h, bp.pad_w, bp.scale = n, self.in_ch, h0, w0, Hp, Wp, self.scale
        bp.dtype = ops.rsa_dtype(dtype)
        bp.out_H, bp.out_W, bp.out_h, bp.out_w = H * s, Wd * s, H * s, Wd * s
        bp.x, bp.out = plan.input_ref(x_shape, dtype).data_ptr(), y.data_ptr()
        plan.launch('rsa_bilinear_add', bp)
        return set_input
