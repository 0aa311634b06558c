"""FIGSR on the MI355X engine (reference module: ``resselt/archs/figsr/arch.py:398-708``), eval-mode semantics.

The gated block is GFISRv2's (``archs/gfisrv2/arch.py``) with dense Inception branches: fc1's output splits into
[g | i | c | c_hw | c_w | c_h] = [hidden, hidden - dim, dim - 3 gc, gc, gc, gc] channels, every split on a plane boundary by construction
(``hidden`` and ``gc`` are multiples of 8), the branches do not rotate, and fc1's rows need no re-layout.  ``c`` goes through the
FourierUnit (GFISRv2's, value for value: ``engine/fourier.py``), ``c_hw`` through a dense gc -> gc square convolution, ``c_w`` / ``c_h`` through dense gc -> gc
1 x K / K x 1 bands.  There is no activation behind fc2 and no gamma: the block is ``fc2(silu(g) * cat(...)) + x``.  Per block, nine
launches:

  rsa_rmsnorm -> fc1 3x3 -> rsa_gfisr_dft (rfft2 of the ``c`` planes -> an f32 spectral map, [real | imag])
  -> rsa_gfisr_spectral (rn + fpe + its residual -> bf16 split planes) -> fdc 1x1 + GELU (three bf16 products in every policy, f32 map)
  -> rsa_gfisr_dft (irfft2 + post_norm, back into the ``c`` planes) -> rsa_plk_conv (convhw on the ``c_hw`` planes, into scratch planes)
  -> rsa_figsr_mix (both bands on the MFMA and silu(g) * cat(i, c, hw, w, h) in one launch) -> fc2 3x3 with the block's residual

fdc's output rows are reordered from the reference's interleaved (re, im) pairs to [real of all | imag of all].  The reference's RMSNorm
reads ``eps`` and ``rms`` from the checkpoint (``x / (eps + ||x|| rms)``): with k = rms sqrt(C) that is ``(x / k) / (eps / k + ||x|| /
sqrt(C))``, so the kernels' form takes ``scale / k`` and ``eps / k`` (k = 1 for every checkpoint the reference writes).

Around the trunk: ``(x - shift) / scale_norm`` and the reflect pad (4, 4 + W % 2, 4, 4 + H % 2) in one kernel (rsa_figsr_input; the affine
is NOT folded into in_to_dim, whose zero padding pads the normalised image), in_to_dim 3x3, ``n // 2`` blocks (-> x0), ``n - n // 2``
blocks and a 3x3 convolution (-> x1), cat_to_dim 1x1 over the planes [x1 | x | x0] (their producers write straight into one buffer),
UniUpsampleV3 through ``engine/uniupsample.py`` into an f32 map of the padded size, then the crop and ``* scale_norm + shift`` in one kernel
(rsa_figsr_output).  The DFT tables are built once per plan for the padded size.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import lib_figsr as LF
from ...engine import ops, plk
from ...engine.base import Plan, check_fp16_range
from ...engine.fourier import EPS, dft_workspace, emit_fourier_unit, pack_fourier_unit
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ...engine.uniupsample import SAMPLE_MODS, SAMPLE_MODS3, Head, OwnMetaUpsample
from ..mosr.arch import _check_dims, _conv_weights, _GatedBase

MAX_CF = 128  # rsa_gfisr_dft: at most 128 channels per transform
EXTRA = 4  # the reflect pad on every side (arch.py:675)
HALVES = ('gfisr_body_half', 'gfisr_body_half_2')


class FIGSR(OwnMetaUpsample, _GatedBase):  # (the reference's load_state_dict override: arch.py:666-668)
    rms_norm = True
    global_statistics = True  # the FourierUnit spans the whole tensor it is given: a tile computes what the reference computes on that tile

    def __init__(self, in_nc: int = 3, dim: int = 48, expansion_ratio: float = 8 / 3, scale: int = 4, out_nc: int = 3,
                 upsampler: str = 'pixelshuffledirect', mid_dim: int = 32, n_blocks: int = 24, gc: int = 8, square_kernel_size: int = 13,
                 band_kernel_size: int = 17, hidden: int | None = None, halves: tuple | None = None, **kwargs) -> None:  # fmt: skip
        """``hidden``: the width of fc2's input where a checkpoint gives it (the loader reads it from the ``fc1`` shape); otherwise
        ``int(expansion_ratio * dim) // 8 * 8`` as the reference computes it.  ``halves``: the block counts of the two halves as the
        checkpoint has them; the reference module always builds (n // 2, n - n // 2)."""
        super().__init__()
        if in_nc != 3 or out_nc != 3:
            raise NotImplementedError(f'FIGSR: 3 input and 3 output channels (shift and scale_norm have three; the reference raises in forward for others; got {in_nc}, {out_nc})')
        if dim % 8:
            raise NotImplementedError(f'FIGSR: dim must be a multiple of 8 (got {dim})')
        _check_dims('FIGSR', dim, in_nc)
        if gc not in (8, 16):
            raise NotImplementedError(f'FIGSR: gc must be 8 or 16 (got {gc})')
        cf = dim - 3 * gc
        if cf < 8 or cf > MAX_CF:
            raise NotImplementedError(f'FIGSR: dim - 3 gc must be in 8..{MAX_CF} (got {cf})')
        for what, k in (('square', square_kernel_size), ('band', band_kernel_size)):
            if k < 3 or k > 31 or k % 2 == 0:
                raise NotImplementedError(f'FIGSR: the {what} kernel size must be odd, 3..31 (got {k})')
        if n_blocks < 2:
            raise NotImplementedError('FIGSR: at least two blocks (the reference does not detect a checkpoint with an empty first half)')
        halves = (n_blocks // 2, n_blocks - n_blocks // 2) if halves is None else tuple(int(v) for v in halves)
        if halves != (n_blocks // 2, n_blocks - n_blocks // 2):
            raise NotImplementedError(f'FIGSR: the halves must be the (n // 2, n - n // 2) split of {n_blocks} blocks (got {halves}; the reference module cannot take such a state dict)')
        if upsampler not in SAMPLE_MODS3:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS3}')
        if scale != 1 and upsampler not in SAMPLE_MODS:
            raise NotImplementedError(f'FIGSR: the {upsampler} head is not built (conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample are)')
        hidden = int(expansion_ratio * dim) // 8 * 8 if hidden is None else int(hidden)
        if hidden < dim or hidden % 8:
            raise NotImplementedError(f'FIGSR: hidden = int(expansion_ratio * dim) // 8 * 8 must be a multiple of 8 and at least dim (got {hidden})')
        self.in_ch, self.out_ch, self.scale, self.dim, self.n_block, self.hidden = in_nc, out_nc, scale, dim, n_blocks, hidden
        self.head, self.mid_dim, self.gc, self.cf, self.halves = upsampler, mid_dim, gc, cf, halves
        self.ksq, self.kband = square_kernel_size, band_kernel_size
        self.up = Head('upscale', upsampler, scale, dim, out_nc, mid_dim, end_kernel=3, version=3)
        self.blocks = [f'{HALVES[0]}.{i}' for i in range(halves[0])] + [f'{HALVES[1]}.{i}' for i in range(halves[1])]
        shapes: dict = {'shift': (1, 3, 1, 1), 'scale_norm': (1, 3, 1, 1), 'in_to_dim.weight': (dim, in_nc, 3, 3), 'in_to_dim.bias': (dim,)}

        def rms(name, c):
            shapes[f'{name}.scale'], shapes[f'{name}.offset'], shapes[f'{name}.eps'], shapes[f'{name}.rms'] = (c,), (c,), (1,), (1,)

        for b in self.blocks:
            rms(f'{b}.norm', dim)
            shapes[f'{b}.fc1.weight'], shapes[f'{b}.fc1.bias'] = (2 * hidden, dim, 3, 3), (2 * hidden,)
            fu = f'{b}.conv.fu'
            rms(f'{fu}.rn', 2 * cf)
            rms(f'{fu}.post_norm', cf)
            shapes[f'{fu}.fdc.weight'], shapes[f'{fu}.fdc.bias'] = (2 * cf, 2 * cf, 1, 1), (2 * cf,)
            shapes[f'{fu}.fpe.weight'], shapes[f'{fu}.fpe.bias'] = (2 * cf, 1, 3, 3), (2 * cf,)
            shapes[f'{b}.conv.convhw.weight'], shapes[f'{b}.conv.convhw.bias'] = (gc, gc, self.ksq, self.ksq), (gc,)
            shapes[f'{b}.conv.convw.weight'], shapes[f'{b}.conv.convw.bias'] = (gc, gc, 1, self.kband), (gc,)
            shapes[f'{b}.conv.convh.weight'], shapes[f'{b}.conv.convh.bias'] = (gc, gc, self.kband, 1), (gc,)
            shapes[f'{b}.fc2.weight'], shapes[f'{b}.fc2.bias'] = (dim, hidden, 3, 3), (dim,)
        t = f'{HALVES[1]}.{halves[1]}'
        shapes[f'{t}.weight'], shapes[f'{t}.bias'] = (dim, dim, 3, 3), (dim,)
        shapes['cat_to_dim.weight'], shapes['cat_to_dim.bias'] = (dim, 3 * dim, 1, 1), (dim,)
        buffers: dict = {}
        self.up.shapes(shapes, buffers, whole_planes='FIGSR')
        build_param_tree(self, shapes, buffers)
        with torch.no_grad():  # the reference's initial values: a module built without a checkpoint normalises as the reference's does
            self.shift.fill_(0.5)
            self.scale_norm.fill_(1 / 6)
            for name, p in self.named_parameters():
                if name.endswith('.eps'):
                    p.fill_(EPS)
                elif name.endswith('.rms'):
                    p.fill_(p_dim(self, name) ** -0.5)
                elif name.endswith('.scale'):
                    p.fill_(1.0)

    # ---------------------------------------------------------------- weights
    @staticmethod
    def _rms(sd, name, c):
        """(scale / k, offset, eps / k) of the RMSNorm ``name`` over ``c`` channels: the kernels' form of the reference's
        ``x / (eps + ||x|| rms)`` (k = rms sqrt(c), 1 for the reference's own checkpoints)."""
        k = float(sd[f'{name}.rms'].reshape(-1)[0]) * c**0.5
        eps = float(sd[f'{name}.eps'].reshape(-1)[0])
        if not k > 0.0 or not eps > 0.0:
            raise NotImplementedError(f'FIGSR: {name}.rms and {name}.eps must be positive (got {k / c**0.5}, {eps})')
        return (sd[f'{name}.scale'].reshape(-1) / k).contiguous(), sd[f'{name}.offset'].reshape(-1).contiguous(), eps / k

    def _pack_block(self, W, sd, b, products, device):
        dim, cf = self.dim, self.cf
        blk = {'norm': self._rms(sd, f'{b}.norm', dim)}
        # rsa_rmsnorm writes bf16 planes: in the fp16 mode fc1 reads them in one bf16 product
        blk['fc1'] = ops.ConvWeights.from_oihw(sd[f'{b}.fc1.weight'], sd[f'{b}.fc1.bias'], products if products.fmt == PF_BF16 else 1, fmt=PF_BF16, device=device)
        blk['fc2'] = ops.ConvWeights.from_oihw(sd[f'{b}.fc2.weight'], sd[f'{b}.fc2.bias'], products, device=device)
        fu = f'{b}.conv.fu'
        blk.update(pack_fourier_unit(sd, fu, cf, self._rms(sd, f'{fu}.rn', 2 * cf), self._rms(sd, f'{fu}.post_norm', cf), device))
        c = f'{b}.conv'
        blk['hw'] = (plk.pack_plk_weights(sd[f'{c}.convhw.weight'], int(products), products.fmt), plk.plk_bias(sd[f'{c}.convhw.bias']))
        blk['band'] = (LF.pack_band_weights(sd[f'{c}.convw.weight'], sd[f'{c}.convh.weight'], int(products), products.fmt),
                       LF.band_bias(sd[f'{c}.convw.bias']), LF.band_bias(sd[f'{c}.convh.bias']))  # fmt: skip
        W[b] = blk

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
        W: dict = {'conv0': cw(sd['in_to_dim.weight'], sd['in_to_dim.bias'])}
        for b in self.blocks:
            self._pack_block(W, sd, b, products, device)
        t = f'{HALVES[1]}.{self.halves[1]}'
        W['tail'] = cw(sd[f'{t}.weight'], sd[f'{t}.bias'])
        W['cat'] = cw(sd['cat_to_dim.weight'], sd['cat_to_dim.bias'])
        W['shift'], W['scale_norm'] = sd['shift'].reshape(-1).contiguous(), sd['scale_norm'].reshape(-1).contiguous()
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        """Convolution MACs per pixel of the padded map; the dense DFT is not a per-pixel cost (O(H + W) per pixel) and is left out."""
        d, h, cf, gc = self.dim, self.hidden, self.cf, self.gc
        blk = 9 * d * 2 * h + (self.ksq**2 + 2 * self.kband) * gc * gc + 9 * h * d + 2 * cf * 2 * cf + 9 * 2 * cf
        return 9 * self.in_ch * d + self.n_block * blk + 9 * d * d + 3 * d * d + self.up.macs()

    # ---------------------------------------------------------------- plan
    def _emit_block(self, plan: Plan, blk, n, H, Wd, cur, bufs):
        N_pl, F_pl, M_pl, HW_pl = (bufs[k] for k in ('norm', 'fc1', 'gate', 'hw'))
        cf, gc = self.cf, self.gc
        hp, P = self.hidden // 8, gc // 8
        i_pl, f_pl = (self.hidden - self.dim) // 8, cf // 8
        products = 3 if F_pl.lo is not None else 1
        sc, off, eps = blk['norm']
        plan.launch('rsa_rmsnorm', dict(x_f32=cur, batch=n, H=H, W=Wd, C=self.dim, eps=eps, scale=sc, offset=off, out=N_pl))
        plan.conv(ops.conv_params(blk['fc1'], N_pl, H, Wd, out=F_pl))
        emit_fourier_unit(plan, blk, bufs['dft'], n, H, Wd, cf, F_pl, hp + i_pl, bufs['spec'], bufs['sp'])
        # convhw reads the c_hw planes of fc1's output and writes scratch planes: rsa_plk_conv has no in-place form
        c0 = hp + i_pl + f_pl
        src = Planes(F_pl.hi[:, c0 : c0 + P], None if F_pl.lo is None else F_pl.lo[:, c0 : c0 + P])
        unit = 16 * (2 if F_pl.lo is not None else 1)
        kp = plk.plk_params(blk['hw'][0], blk['hw'][1], self.ksq, products, src, HW_pl, 0)
        plan.launch('rsa_plk_conv', kp, meta=dict(kernel='rsa_plk_conv', flop=2 * n * H * Wd * gc * gc * self.ksq**2, bytes=n * H * Wd * unit * 2 * P))
        mp = LF.FigsrMixParams()
        mp.batch, mp.H, mp.W, mp.fmt, mp.products, mp.ksize, mp.gc = n, H, Wd, F_pl.fmt, products, self.kband, gc
        mp.planes, mp.pass_planes = hp, i_pl + f_pl
        mp.w_packed, mp.bias_w, mp.bias_h = (t.data_ptr() for t in blk['band'])
        F_pl.bind(mp, 'g')
        F_pl.bind(mp, 'x', hp)
        HW_pl.bind(mp, 'hw')
        M_pl.bind(mp, 'out')
        # byte model: g, cat(i, c, c_w, c_h) and hw read once, the product written once (the band halos stay on chip); the bands' 2 K gc^2
        # MACs per pixel are a small fraction of a stream of 3 hidden / 8 units per pixel: priced by its bytes, like the gate it replaces
        plan.launch('rsa_figsr_mix', mp, meta=dict(kernel='rsa_figsr_mix', flop=0, bytes=n * H * Wd * unit * 3 * hp))
        return M_pl

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        if h0 < EXTRA + 2 or w0 < EXTRA + 2:
            # the reference's F.pad raises: the reflection of EXTRA + size % 2 pixels needs more than that many (5 x 5, 5 x 6 and 4 x 8 raise, 6 x 6 runs)
            raise RuntimeError(f'Padding size should be less than the corresponding input dimension (a {h0}x{w0} input: FIGSR needs at least {EXTRA + 2} pixels in either direction)')
        s, dim, cf, gc = self.scale, self.dim, self.cf, self.gc
        H, Wd = h0 + 2 * EXTRA + h0 % 2, w0 + 2 * EXTRA + w0 % 2
        pd, hp = dim // 8, self.hidden // 8
        Wf = Wd // 2 + 1
        with_lo = products == 3
        dev = plan.device
        x_pl = plan.planes(n, 1, H, Wd, with_lo)
        ip = LF.FigsrInputParams()
        ip.batch, ip.C, ip.src_h, ip.src_w, ip.pad, ip.dtype, ip.fmt = n, c, h0, w0, EXTRA, ops.rsa_dtype(dtype), x_pl.fmt
        ip.shift, ip.scale_norm = W['shift'].data_ptr(), W['scale_norm'].data_ptr()
        x_pl.bind(ip, 'out')

        def set_input(x):
            ip.x = x.data_ptr()
            L.launch('rsa_figsr_input', ip, ops.current_stream_ptr(dev))  # the affine and the reflect pad, fused

        T, S0, S1 = (plan.f32map(n, dim, H, Wd) for _ in range(3))  # in_to_dim's output, and the stream
        cat_pl = plan.planes(n, 3 * pd, H, Wd, with_lo)  # [x1 | x | x0]: what cat_to_dim reads
        feat = plan.planes(n, pd, H, Wd, with_lo)
        bufs = dict(norm=plan.planes(n, pd, H, Wd, with_lo, fmt=PF_BF16), fc1=plan.planes(n, 2 * hp, H, Wd, with_lo), gate=plan.planes(n, hp, H, Wd, with_lo),
                    hw=plan.planes(n, gc // 8, H, Wd, with_lo), spec=plan.f32map(n, 2 * cf, H, Wf), sp=plan.planes(n, (2 * cf + 7) // 8, H, Wf, True, fmt=PF_BF16),
                    dft=dft_workspace(plan, 'FIGSR', n, cf, H, Wd))  # fmt: skip
        plan.conv(ops.conv_params(W['conv0'], x_pl, H, Wd, out=cat_pl, out_plane_off=pd, out_f32=T))
        cur, nxt = T, S0
        for i, b in enumerate(self.blocks):
            m = self._emit_block(plan, W[b], n, H, Wd, cur, bufs)
            if i == self.halves[0] - 1:  # x0: the stream goes on, and cat_to_dim reads it
                plan.conv(ops.conv_params(W[b]['fc2'], m, H, Wd, res1=cur, alpha=1.0, out=cat_pl, out_plane_off=2 * pd, out_f32=nxt))
            elif i == self.n_block - 1:  # the 3x3 convolution behind the second half reads planes
                plan.conv(ops.conv_params(W[b]['fc2'], m, H, Wd, res1=cur, alpha=1.0, out=feat))
            else:
                plan.conv(ops.conv_params(W[b]['fc2'], m, H, Wd, res1=cur, alpha=1.0, out_f32=nxt))
            cur, nxt = nxt, (S1 if nxt is S0 else S0)
        plan.conv(ops.conv_params(W['tail'], feat, H, Wd, out=cat_pl))
        fe = plan.planes(n, pd, H, Wd, with_lo)
        fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None
        plan.conv(ops.conv_params(W['cat'], cat_pl, H, Wd, out=fe, out_f32=fe32))
        full = torch.empty((n, self.out_ch, H * s, Wd * s), dtype=torch.float32, device=dev)  # the head's result at the padded size
        plan.keep.append(full)
        self.up.emit(plan, W, fe, fe32, full, with_lo)
        y = plan.output((n, self.out_ch, h0 * s, w0 * s), dtype)
        op = LF.FigsrOutputParams()
        op.batch, op.C, op.H, op.W, op.y0, op.x0, op.out_h, op.out_w, op.dtype = n, self.out_ch, H * s, Wd * s, EXTRA * s, EXTRA * s, h0 * s, w0 * s, ops.rsa_dtype(dtype)
        op.y, op.shift, op.scale_norm, op.out = full.data_ptr(), W['shift'].data_ptr(), W['scale_norm'].data_ptr(), y.data_ptr()
        plan.launch('rsa_figsr_output', op)
        return set_input


def p_dim(module, name: str) -> int:
    """The channel count of the RMSNorm that owns parameter ``name`` (``....rms``): the length of its ``scale``."""
    return module.get_parameter(name[: -len('rms')] + 'scale').numel()
