"""GFISR (v1) on the MI355X engine (reference module: ``resselt/archs/gfisr/arch.py:385-629``), eval-mode semantics.

The model GFISRv2, FIGSR and LAWFFT descend from.  Its gated block is MoSR's (``archs/mosr/arch.py``, shared through ``_GatedBase``): a
centred channel LayerNorm, a Mish gate, Mish behind fc2.  The Inception step has FIVE modules -- identity (dim - 4 gc channels), dw 3x3,
dw 1x11, dw 11x1 and a ``FourierUnit`` (gc = dim / 8 channels each) -- and every block holds all five; attribute names and channel positions
rotate with ``shift % 5``.  In eval mode the FourierUnit reflect-pads its input by 2 on every side (one more row / column at the bottom /
right of an odd side), transforms the padded image and crops the result; between the transforms it runs a channel LayerNorm over the 2 gc
spectral channels, fpe with its residual, and fdc + GELU.  Its ``weight`` branch (a 1x1 convolution to ONE channel and a softmax over that
channel) is exactly 1.0 for every finite input: the two tensors are parameters of the tree and take no part in the arithmetic.
Per block, ten launch steps (twelve kernels: a transform is two):

  rsa_layernorm (f32 stream -> planes) -> fc1 3x3 -> rsa_plane_window (the reflect pad of the Fourier branch's planes of fc1's output)
  -> rsa_gfisr_dft (rfft2 at (Hp, Wp) -> an f32 spectral map, [real | imag]) -> rsa_gfisr_ln_spectral (ln + fpe + residual + fdc + GELU, f32)
  -> rsa_gfisr_dft (irfft2, no norm, back into the padded planes) -> rsa_plane_window (the crop, into the Fourier planes of fc1's output)
  -> rsa_gated_dwconv (mish(g) * cat(i, c); passthrough [i | identity | Fourier], segments 3x3, 1x11, 11x1) -> fc2 3x3 + Mish
  -> rsa_group_norm_apply (x * gamma + shortcut)

With ``fft_mode=False`` the fifth module is an identity: the five Fourier steps are dropped and its planes stay part of the passthrough.
At pack time fc1's rows are re-laid out so that every branch starts on a plane boundary whatever its rotated position
(``gfisr1_gate_layout``), and ln, fpe and both sides of fdc are permuted from the reference's interleaved (re, im) channel pairs to
[real of all | imag of all], the order both transforms use (LayerNorm's statistics do not depend on the order).

The DFT tables depend on (Hp, Wp) alone; ``_build_plan`` builds them once per plan.  Trunk: in_to_dim 3x3, the blocks, + in_to_dim's output
(no tail convolutions).  ``pixel_unshuffle`` with scale 1 or 2 puts PadPixelUnshuffle(4 // scale) in front (fused into the input
conversion) and runs the head at x4; the output is cropped to (h scale, w scale).  Head: UniUpsampleV3 as in GFISRv2.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import lib_gfisr1 as LG1
from ...engine import ops, plk
from ...engine.base import Plan, check_fp16_range
from ...engine.fourier import EPS, dft_workspace, emit_dft
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16
from ...engine.uniupsample import SAMPLE_MODS, SAMPLE_MODS3, Head, OwnMetaUpsample
from ..mosr.arch import _check_dims, _conv_weights, _GatedBase, pad_dw, relayout_gate

MAX_DIM = 128  # gc = dim / 8 <= 16: rsa_gfisr_ln_spectral takes at most 32 spectral channels
FIXED_MID_DIM = 32  # what the reference's loader always builds (it hands ``upsample_dim=`` to a constructor whose parameter is ``mid_dim``)
SLOTS = ('pconv', 'dwconv_hw', 'dwconv_w', 'dwconv_h', 'fsas')  # InceptionDWConv2d's attribute names, in channel order
KINDS = ('identity', (3, 3), (1, 11), (11, 1), 'fourier')  # the five modules before rotation
PAD = 2  # the FourierUnit's reflect pad on every side (+ one row / column at the bottom / right of an odd side)


def branch_order(shift: int):
    """[(attribute name, 'identity' | 'fourier' | kernel shape)] of block ``shift`` in channel order (gfisr/arch.py:508-520)."""
    return [(SLOTS[t], KINDS[(shift + t) % 5]) for t in range(5)]


def gfisr1_gate_layout(hidden: int, dim: int, shift: int):
    """Plane layout of cat(i, c) for block ``shift``: [i | identity | FourierUnit | the three depthwise segments in channel order], each from
    a plane boundary.  Returns (perm, i_planes, d_planes, f_planes, segments, planes): perm[j] the padded position of reference channel j,
    segments [(planes, kh, kw, attribute name)]."""
    gc = dim // 8
    idc = dim - 4 * gc
    i_ch = hidden - dim
    i_pl, d_pl, g_pl = (i_ch + 7) // 8, (idc + 7) // 8, (gc + 7) // 8
    perm = list(range(i_ch))
    d0, f0 = 8 * i_pl, 8 * (i_pl + d_pl)
    pos = 8 * (i_pl + d_pl + g_pl)
    segs = []
    for name, kind in branch_order(shift):
        if kind == 'identity':
            perm += list(range(d0, d0 + idc))
        elif kind == 'fourier':
            perm += list(range(f0, f0 + gc))
        else:
            perm += list(range(pos, pos + gc))
            segs.append((g_pl, kind[0], kind[1], name))
            pos += 8 * g_pl
    return perm, i_pl, d_pl, g_pl, segs, pos // 8


def padded_size(H: int, W: int):
    """The size the FourierUnit transforms at (pad_to_even with expand_all_sides, gfisr/arch.py:385-400)."""
    return H + 2 * PAD + H % 2, W + 2 * PAD + W % 2


class GFISR(OwnMetaUpsample, _GatedBase):  # (the reference's load_state_dict override: arch.py:620-623)
    global_statistics = True  # the FourierUnit spans the whole tensor it is given: a tile computes what the reference computes on that tile

    def __init__(self, in_nc: int = 3, dim: int = 48, expansion_ratio: float = 8 / 3, fft_mode: bool = True, scale: int = 4, out_nc: int = 3,
                 upsampler: str = 'pixelshuffledirect', mid_dim: int = 32, pixel_unshuffle: bool = True, n_blocks: int = 24,
                 hidden: int | None = None, **kwargs) -> None:  # fmt: skip
        """``hidden``: the width of fc2's input where a checkpoint gives it (the loader reads it from the ``fc1`` shape); otherwise
        ``int(expansion_ratio * dim)`` as the reference computes it."""
        super().__init__()
        if dim % 8 or dim > MAX_DIM:
            raise NotImplementedError(f'GFISR: dim must be a multiple of 8 up to {MAX_DIM} (got {dim})')
        _check_dims('GFISR', dim, in_nc)
        if out_nc < 1 or out_nc > 8:
            raise NotImplementedError(f'GFISR: 1 to 8 output channels are built (got {out_nc})')
        if n_blocks < 1:
            raise NotImplementedError('GFISR: at least one block')
        if upsampler not in SAMPLE_MODS3:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS3}')
        self.unshuffle = 4 // scale if pixel_unshuffle and scale in (1, 2) else 1
        s_head = 4 if self.unshuffle > 1 else scale
        if s_head != 1 and upsampler not in SAMPLE_MODS:
            raise NotImplementedError(f'GFISR: the {upsampler} head is not built (conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample are)')
        hidden = int(expansion_ratio * dim) if hidden is None else int(hidden)
        if hidden < dim:
            raise NotImplementedError(f'GFISR: hidden = int(expansion_ratio * dim) must be at least dim (got {hidden})')
        self.in_ch, self.out_ch, self.dim, self.n_block, self.hidden = in_nc, out_nc, dim, n_blocks, hidden
        self.out_scale, self.scale = scale, s_head  # ``scale``: the head's; ``out_scale``: the model's
        self.head, self.mid_dim, self.gc, self.fft_mode = upsampler, mid_dim, dim // 8, bool(fft_mode)
        self.up = Head('dim_to_out', upsampler, s_head, dim, out_nc, mid_dim, end_kernel=3, version=3)
        gc, u = self.gc, self.unshuffle
        first = 'in_to_dim.1' if u > 1 else 'in_to_dim'
        shapes: dict = {f'{first}.weight': (dim, in_nc * u * u, 3, 3), f'{first}.bias': (dim,)}
        for i in range(n_blocks):
            b = f'net.{i}'
            shapes[f'{b}.gamma'] = (1, dim, 1, 1)
            shapes[f'{b}.norm.weight'], shapes[f'{b}.norm.bias'] = (dim,), (dim,)
            shapes[f'{b}.fc1.weight'], shapes[f'{b}.fc1.bias'] = (2 * hidden, dim, 3, 3), (2 * hidden,)
            for name, kind in branch_order(i):
                c = f'{b}.conv.{name}'
                if kind == 'fourier' and self.fft_mode:
                    shapes[f'{c}.ln.weight'], shapes[f'{c}.ln.bias'] = (2 * gc,), (2 * gc,)
                    shapes[f'{c}.fdc.weight'], shapes[f'{c}.fdc.bias'] = (2 * gc, 2 * gc, 1, 1), (2 * gc,)
                    shapes[f'{c}.weight.0.weight'], shapes[f'{c}.weight.0.bias'] = (1, 2 * gc, 1, 1), (1,)  # the dead softmax branch
                    shapes[f'{c}.fpe.weight'], shapes[f'{c}.fpe.bias'] = (2 * gc, 1, 3, 3), (2 * gc,)
                elif isinstance(kind, tuple):
                    shapes[f'{c}.weight'], shapes[f'{c}.bias'] = (gc, 1, *kind), (gc,)
            shapes[f'{b}.fc2.weight'], shapes[f'{b}.fc2.bias'] = (dim, hidden, 3, 3), (dim,)
        buffers: dict = {}
        self.up.shapes(shapes, buffers, whole_planes='GFISR')
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack_block(self, W, sd, b, products, device):
        shift = int(b.rsplit('.', 1)[1])
        dim, gc = self.dim, self.gc
        perm, i_pl, d_pl, f_pl, segs, planes = gfisr1_gate_layout(self.hidden, dim, shift)
        w1, b1, w2 = relayout_gate(sd[f'{b}.fc1.weight'], sd[f'{b}.fc1.bias'], sd[f'{b}.fc2.weight'], perm, planes)
        f32 = torch.float32
        blk = {'norm': (sd[f'{b}.norm.weight'].contiguous(), sd[f'{b}.norm.bias'].contiguous())}
        blk['fc1'] = ops.ConvWeights.from_oihw(w1.to(f32), b1.to(f32), products, device=device)
        blk['fc2'] = ops.ConvWeights.from_oihw(w2.to(f32), sd[f'{b}.fc2.bias'], products, device=device)
        blk['segs'] = [(pl, kh, kw, *pad_dw(sd[f'{b}.conv.{name}.weight'], sd[f'{b}.conv.{name}.bias'], pl)) for pl, kh, kw, name in segs]
        blk['i_planes'], blk['f0'], blk['f_planes'], blk['planes'] = i_pl + d_pl + f_pl, i_pl + d_pl, f_pl, planes
        blk['gamma'] = sd[f'{b}.gamma'].reshape(-1).contiguous()
        if self.fft_mode:
            fu = f'{b}.conv.{next(name for name, kind in branch_order(shift) if kind == "fourier")}'
            # reference channel 2k is the real part of k and 2k + 1 its imaginary part, on both sides of ln, fpe and fdc: stored as
            # [real of all | imag of all]
            rows = torch.cat([torch.arange(0, 2 * gc, 2), torch.arange(1, 2 * gc, 2)]).to(device)
            own = lambda t: t.to(f32).contiguous().clone()  # noqa: E731  (an allocation of its own: 16-byte aligned)
            blk['ln'] = (own(sd[f'{fu}.ln.weight'][rows]), own(sd[f'{fu}.ln.bias'][rows]))
            blk['fpe'] = (own(sd[f'{fu}.fpe.weight'].reshape(2 * gc, 9)[rows]), own(sd[f'{fu}.fpe.bias'][rows]))
            blk['fdc'] = (own(sd[f'{fu}.fdc.weight'].reshape(2 * gc, 2 * gc)[rows][:, rows]), own(sd[f'{fu}.fdc.bias'][rows]))
        W[b] = blk

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        first = 'in_to_dim.1' if self.unshuffle > 1 else 'in_to_dim'
        W: dict = {'conv0': ops.ConvWeights.from_oihw(sd[f'{first}.weight'], sd[f'{first}.bias'], products, device=device)}
        for i in range(self.n_block):
            self._pack_block(W, sd, f'net.{i}', products, device)
        W['zeros'] = torch.zeros(self.dim, dtype=torch.float32, device=device)
        W['ones'] = torch.ones(self.dim, dtype=torch.float32, device=device)
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        """Convolution and depthwise MACs per input pixel; the dense DFT is not a per-pixel cost (O(H + W) per pixel) and is left out."""
        d, h, gc, u = self.dim, self.hidden, self.gc, self.unshuffle
        blk = 9 * d * 2 * h + (9 + 22) * gc + 9 * h * d + (2 * gc * 2 * gc + 9 * 2 * gc if self.fft_mode else 0)
        return (9 * self.in_ch * u * u * d + self.n_block * blk + self.up.macs()) // (u * u)

    # ---------------------------------------------------------------- plan
    def _window(self, plan: Plan, n, src, src0, H, Wd, dst, dst0, out_H, out_W, top, left, planes) -> None:
        wp = LG1.PlaneWindowParams()
        wp.batch, wp.planes, wp.H, wp.W, wp.out_H, wp.out_W, wp.top, wp.left = n, planes, H, Wd, out_H, out_W, top, left
        src.bind(wp, 'in', src0)
        dst.bind(wp, 'out', dst0)
        if wp.in_lo is None or wp.out_lo is None:
            wp.in_lo = wp.out_lo = None
        unit = 16 * (2 if wp.out_lo is not None else 1)
        plan.launch('rsa_plane_window', wp, meta=dict(kernel='rsa_plane_window', flop=0, bytes=2 * n * planes * out_H * out_W * unit,
                                                       label='reflect pad' if top > 0 else 'crop'))  # fmt: skip

    def _emit_branches(self, plan: Plan, blk, n, H, Wd, bufs) -> None:
        """The FourierUnit on the Fourier branch's planes of fc1's output, in place (``fft_mode``; otherwise they are an identity's)."""
        if not self.fft_mode:
            return
        F_pl, P_pl, spec, spec2, dft = (bufs[k] for k in ('fc1', 'pad', 'spec', 'spec2', 'dft'))
        Hp, Wp = padded_size(H, Wd)
        Wf = Wp // 2 + 1
        f0, f_pl = blk['planes'] + blk['f0'], blk['f_planes']
        self._window(plan, n, F_pl, f0, H, Wd, P_pl, 0, Hp, Wp, PAD, PAD, f_pl)
        emit_dft(plan, dft, False, n, self.gc, Hp, Wp, spec, P_pl, 0)
        sp = LG1.GfisrLnSpectralParams()
        sp.batch, sp.H, sp.W, sp.C, sp.eps = n, Hp, Wf, 2 * self.gc, EPS
        sp.x, sp.out = spec.data_ptr(), spec2.data_ptr()
        sp.ln_w, sp.ln_b = (t.data_ptr() for t in blk['ln'])
        sp.fpe_w, sp.fpe_b = (t.data_ptr() for t in blk['fpe'])
        sp.fdc_w, sp.fdc_b = (t.data_ptr() for t in blk['fdc'])
        c2 = 2 * self.gc
        # byte model: the f32 map read once (the halo re-reads stay on chip) and written once
        plan.launch('rsa_gfisr_ln_spectral', sp, meta=dict(kernel='rsa_gfisr_ln_spectral', flop=2 * n * Hp * Wf * (c2 * c2 + 10 * c2), bytes=n * Hp * Wf * 2 * c2 * 4))
        emit_dft(plan, dft, True, n, self.gc, Hp, Wp, spec2, P_pl, 0)
        self._window(plan, n, P_pl, 0, Hp, Wp, F_pl, f0, H, Wd, -PAD, -PAD, f_pl)

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        u, s, dim, gc = self.unshuffle, self.scale, self.dim, self.gc
        Hg, Wg = h0 + (u - h0 % u) % u, w0 + (u - w0 % u) % u
        if Hg - h0 >= h0 or Wg - w0 >= w0:
            raise RuntimeError('Padding size should be less than the corresponding input dimension (the input is too small for PadPixelUnshuffle)')
        H, Wd = Hg // u, Wg // u
        if self.fft_mode and any(side < 4 or (side % 2 and side < 5) for side in (H, Wd)):
            # the FourierUnit's reflect pad: 2 at the top / left, 2 + side % 2 at the bottom / right, each of which must stay below the side
            raise RuntimeError(f'Padding size should be less than the corresponding input dimension (a {H}x{Wd} feature grid: the reference '
                               'raises in the FourierUnit\'s reflect pad; sides of at least 4, odd sides of at least 5)')  # fmt: skip
        pd = dim // 8
        with_lo = products == 3
        dev = plan.device
        x_pl = plan.planes(n, (self.in_ch * u * u + 7) // 8, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl, unshuffle=u)  # PadPixelUnshuffle's bottom / right reflect pad and the unshuffle, fused

        trunk, S0, S1, R = (plan.f32map(n, dim, H, Wd) for _ in range(4))  # in_to_dim's output (the trunk residual), the stream, fc2 + Mish
        hp = W['net.0']['planes']
        bufs = dict(norm=plan.planes(n, pd, H, Wd, with_lo), fc1=plan.planes(n, 2 * hp, H, Wd, with_lo), gate=plan.planes(n, hp, H, Wd, with_lo))
        if self.fft_mode:
            Hp, Wp = padded_size(H, Wd)
            bufs.update(pad=plan.planes(n, (gc + 7) // 8, Hp, Wp, with_lo), spec=plan.f32map(n, 2 * gc, Hp, Wp // 2 + 1),
                        spec2=plan.f32map(n, 2 * gc, Hp, Wp // 2 + 1), dft=dft_workspace(plan, 'GFISR', n, gc, Hp, Wp))  # fmt: skip
        stats = self._unit_stats(n, dev)
        plan.keep.append(stats)
        plan.conv(ops.conv_params(W['conv0'], x_pl, H, Wd, out_f32=trunk))
        cur, nxt = trunk, S0
        for i in range(self.n_block):
            blk = W[f'net.{i}']
            m = self._emit_block(plan, blk, n, H, Wd, cur, bufs)
            plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, act=L.ACT_MISH, out_f32=R))
            plan.launch('rsa_group_norm_apply', plk.group_norm_apply_params(R, dim, 1, stats, blk['gamma'], W['zeros'], cur, None, nxt))
            cur, nxt = nxt, (S1 if nxt is S0 else S0)
        # net(x) + x: the stream plus in_to_dim's output, as the planes the head reads
        fe = plan.planes(n, pd, H, Wd, with_lo)
        fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None
        plan.launch('rsa_group_norm_apply', plk.group_norm_apply_params(cur, dim, 1, stats, W['ones'], W['zeros'], trunk, fe, fe32))
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * self.out_scale, w0 * self.out_scale))
        self.up.emit(plan, W, fe, fe32, y, with_lo)
        return set_input
