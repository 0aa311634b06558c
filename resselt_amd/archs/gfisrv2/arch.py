"""GFISRv2 on the MI355X engine (reference module: ``resselt/archs/gfisrv2/arch.py:434-686``), eval-mode semantics.

The gated block is MoSRv2's (``archs/mosrv2/arch.py``, shared through ``_GatedBase``) with torch-form RMSNorm, a SiLU gate and a
``FourierUnit`` where the Inception step had its identity branch; the four branches [FourierUnit (cf = dim - 3 gc channels), dw 3x3, dw 1x11,
dw 11x1 (gc = dim / 8 each)] rotate with the block index, attribute names included.  Per block, nine launches:

  rsa_rmsnorm -> fc1 3x3 -> rsa_gfisr_dft (rfft2: the Fourier branch's planes of fc1's output -> an f32 spectral map, [real | imag])
  -> rsa_gfisr_spectral (rn + fpe + its residual -> bf16 split planes) -> fdc 1x1 + GELU (three bf16 products in every policy, f32 map)
  -> rsa_gfisr_dft (irfft2 + post_norm, back into the same planes of fc1's output) -> rsa_gfisr_gate (silu(g) * cat(i, c))
  -> fc2 3x3 + SiLU -> rsa_group_norm_apply (x * gamma + shortcut)

At pack time fc1's rows are re-laid out so that every branch starts on a plane boundary and the Fourier branch sits right behind ``i``
whatever its reference position: to the gate kernel it is part of the passthrough range, whose planes hold post_norm's output by then.
fdc's output rows are reordered from the reference's interleaved (re, im) pairs to [real of all | imag of all], the order both transforms use.
Spectral values stay f32 until rn in every precision policy.

The DFT tables depend on (H, W) alone; ``_build_plan`` builds them once per plan (a plan is cached per input size) in float64.
Trunk: in_to_dim 3x3, the blocks, conv dim -> 2 dim + SiLU, conv 2 dim -> dim, + in_to_dim's output.  No padding anywhere: H and W are
arbitrary.  Head: UniUpsampleV3's conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample (3x3 end convolution) through
``engine/uniupsample.py``; transpose+conv, lda and pa_up are refused.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import lib_gfisr as LG
from ...engine import ops, plk
from ...engine.base import Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ...engine.uniupsample import SAMPLE_MODS, emit_head, head_layers, head_shapes, pack_head
from ..mosr.arch import _check_dims, _conv_weights, _GatedBase, pad_dw, relayout_gate

SAMPLE_MODS3 = SAMPLE_MODS + ('transpose+conv', 'lda', 'pa_up')
MAX_DIM = 128  # rsa_gfisr_dft: at most 128 channels per transform
EPS = 1e-6
GROUPS = 4  # DySample
SLOTS = ('pconv', 'dwconv_hw', 'dwconv_w', 'dwconv_h')  # InceptionDWConv2d's attribute names, in channel order
KINDS = (None, (3, 3), (1, 11), (11, 1))  # the four modules before rotation: None = FourierUnit


def branch_order(shift: int):
    """[(attribute name, kernel shape or None for the FourierUnit)] of block ``shift`` in channel order (gfisrv2/arch.py:536-547)."""
    return [(SLOTS[t], KINDS[(shift + t) % 4]) for t in range(4)]


def gfisr_gate_layout(hidden: int, dim: int, shift: int):
    """Plane layout of cat(i, c) for block ``shift``: [i | FourierUnit | the three depthwise segments in channel order], each from a plane
    boundary.  Returns (perm, i_planes, f_planes, segments, planes, f_src): perm[j] the padded position of reference channel j, segments
    [(planes, kh, kw, attribute name)], f_src the FourierUnit's first reference channel within c."""
    gc = dim // 8
    cf = dim - 3 * gc
    i_ch = hidden - dim
    i_pl, f_pl, g_pl = (i_ch + 7) // 8, (cf + 7) // 8, (gc + 7) // 8
    perm = list(range(i_ch))
    pos = 8 * (i_pl + f_pl)
    src, f_src, segs = 0, 0, []
    for name, kind in branch_order(shift):
        if kind is None:
            perm += list(range(8 * i_pl, 8 * i_pl + cf))
            f_src = src
            src += cf
        else:
            perm += list(range(pos, pos + gc))
            segs.append((g_pl, kind[0], kind[1], name))
            pos += 8 * g_pl
            src += gc
    return perm, i_pl, f_pl, segs, pos // 8, f_src


class GFISRV2(_GatedBase):
    rms_norm = True
    global_statistics = True  # the FourierUnit spans the whole tensor it is given: a tile computes what the reference computes on that tile

    def __init__(self, in_nc: int = 3, dim: int = 48, expansion_ratio: float = 8 / 3, scale: int = 4, out_nc: int = 3,
                 upsampler: str = 'pixelshuffledirect', mid_dim: int = 32, pixel_unshuffle: bool = False, n_blocks: int = 24,
                 hidden: int | None = None, **kwargs) -> None:  # fmt: skip
        """``hidden``: the width of fc2's input where a checkpoint gives it (the loader reads it from the ``fc1`` shape); otherwise
        ``int(expansion_ratio * dim)`` as the reference computes it."""
        super().__init__()
        if pixel_unshuffle:
            raise NotImplementedError('GFISRv2: pixel_unshuffle checkpoints are not built (the reference cannot load them either: its '
                                      'MetaUpsample stores scale 4, so the constructor builds a plain in_to_dim and load_state_dict raises)')  # fmt: skip
        if dim % 8 or dim > MAX_DIM:
            raise NotImplementedError(f'GFISRv2: dim must be a multiple of 8 up to {MAX_DIM} (got {dim})')
        _check_dims('GFISRv2', dim, in_nc)
        if out_nc < 1 or out_nc > 8:
            raise NotImplementedError(f'GFISRv2: 1 to 8 output channels are built (got {out_nc})')
        if n_blocks < 1:
            raise NotImplementedError('GFISRv2: at least one block')
        if upsampler not in SAMPLE_MODS3:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS3}')
        if scale != 1 and upsampler not in SAMPLE_MODS:
            raise NotImplementedError(f'GFISRv2: the {upsampler} head is not built (conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample are)')
        hidden = int(expansion_ratio * dim) if hidden is None else int(hidden)
        if hidden < dim:
            raise NotImplementedError(f'GFISRv2: hidden = int(expansion_ratio * dim) must be at least dim (got {hidden})')
        self.in_ch, self.out_ch, self.scale, self.dim, self.n_block, self.hidden = in_nc, out_nc, scale, dim, n_blocks, hidden
        self.head, self.mid_dim, self.gc = upsampler, mid_dim, dim // 8
        self.cf = dim - 3 * self.gc
        self.layers, self.dys_index = head_layers(upsampler, scale, dim, out_nc, mid_dim)
        if any(co % 8 for _, co, _, _ in self.layers[:-1]) or (self.dys_index == 2 and mid_dim % 8):
            raise NotImplementedError('GFISRv2: the head\'s hidden widths must be multiples of 8')
        cf, gc = self.cf, self.gc
        shapes: dict = {'in_to_dim.weight': (dim, in_nc, 3, 3), 'in_to_dim.bias': (dim,)}
        for i in range(n_blocks):
            b = f'gfisr_body.{i}'
            shapes[f'{b}.gamma'] = (1, dim, 1, 1)
            shapes[f'{b}.norm.scale'] = (dim, 1, 1)
            shapes[f'{b}.norm.offset'] = (dim, 1, 1)
            shapes[f'{b}.fc1.weight'], shapes[f'{b}.fc1.bias'] = (2 * hidden, dim, 3, 3), (2 * hidden,)
            for name, kind in branch_order(i):
                c = f'{b}.conv.{name}'
                if kind is None:
                    shapes[f'{c}.rn.scale'], shapes[f'{c}.rn.offset'] = (2 * cf, 1, 1), (2 * cf, 1, 1)
                    shapes[f'{c}.post_norm.scale'], shapes[f'{c}.post_norm.offset'] = (cf, 1, 1), (cf, 1, 1)
                    shapes[f'{c}.fdc.weight'], shapes[f'{c}.fdc.bias'] = (2 * cf, 2 * cf, 1, 1), (2 * cf,)
                    shapes[f'{c}.fpe.weight'], shapes[f'{c}.fpe.bias'] = (2 * cf, 1, 3, 3), (2 * cf,)
                else:
                    shapes[f'{c}.weight'], shapes[f'{c}.bias'] = (gc, 1, *kind), (gc,)
            shapes[f'{b}.fc2.weight'], shapes[f'{b}.fc2.bias'] = (dim, hidden, 3, 3), (dim,)
        t = n_blocks
        shapes[f'gfisr_body.{t}.weight'], shapes[f'gfisr_body.{t}.bias'] = (2 * dim, dim, 3, 3), (2 * dim,)
        shapes[f'gfisr_body.{t + 2}.weight'], shapes[f'gfisr_body.{t + 2}.bias'] = (dim, 2 * dim, 3, 3), (dim,)
        meta = torch.tensor([3, SAMPLE_MODS3.index(upsampler), scale, dim, out_nc, mid_dim, 4], dtype=torch.uint8)
        buffers = {'upscale.MetaUpsample': meta}
        head_shapes(shapes, buffers, 'upscale', self.layers, self.dys_index, scale, dim, out_nc, mid_dim)
        if self.dys_index is not None:  # dysample_end_kernel = 3
            d = f'upscale.{self.dys_index}.end_conv.weight'
            shapes[d] = (*shapes[d][:2], 3, 3)
        build_param_tree(self, shapes, buffers)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # as the reference (arch.py:678-680): the module's own MetaUpsample wins over the checkpoint's
        state_dict = dict(state_dict)
        state_dict['upscale.MetaUpsample'] = self.get_buffer('upscale.MetaUpsample')
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # ---------------------------------------------------------------- weights
    def _pack_block(self, W, sd, b, products, device):
        shift = int(b.rsplit('.', 1)[1])
        dim, cf = self.dim, self.cf
        perm, i_pl, f_pl, segs, planes, f_src = gfisr_gate_layout(self.hidden, dim, shift)
        w1, b1, w2 = relayout_gate(sd[f'{b}.fc1.weight'], sd[f'{b}.fc1.bias'], sd[f'{b}.fc2.weight'], perm, planes)
        f32 = torch.float32
        blk = {'norm': (sd[f'{b}.norm.scale'].reshape(-1).contiguous(), sd[f'{b}.norm.offset'].reshape(-1).contiguous())}
        # rsa_rmsnorm writes bf16 planes: in the fp16 mode fc1 reads them in one bf16 product
        blk['fc1'] = ops.ConvWeights.from_oihw(w1.to(f32), b1.to(f32), products if products.fmt == PF_BF16 else 1, fmt=PF_BF16, device=device)
        blk['fc2'] = ops.ConvWeights.from_oihw(w2.to(f32), sd[f'{b}.fc2.bias'], products, device=device)
        blk['segs'] = [(pl, kh, kw, *pad_dw(sd[f'{b}.conv.{name}.weight'], sd[f'{b}.conv.{name}.bias'], pl)) for pl, kh, kw, name in segs]
        blk['i_planes'], blk['f_planes'], blk['planes'] = i_pl, f_pl, planes
        blk['gamma'] = sd[f'{b}.gamma'].reshape(-1).contiguous()
        fu = f'{b}.conv.{next(name for name, kind in branch_order(shift) if kind is None)}'

        def padded(t, rows):
            out = torch.zeros((rows, *t.shape[1:]), dtype=f32, device=device)
            out[: t.shape[0]] = t
            return out.contiguous()

        sp = 8 * ((2 * cf + 7) // 8)
        blk['rn'] = (padded(sd[f'{fu}.rn.scale'].reshape(-1), sp), padded(sd[f'{fu}.rn.offset'].reshape(-1), sp))
        blk['fpe'] = (padded(sd[f'{fu}.fpe.weight'].reshape(2 * cf, 9), sp), padded(sd[f'{fu}.fpe.bias'], sp))
        blk['post'] = (padded(sd[f'{fu}.post_norm.scale'].reshape(-1), 8 * f_pl), padded(sd[f'{fu}.post_norm.offset'].reshape(-1), 8 * f_pl))
        # fdc's output row 2k is the real part of channel k and 2k + 1 its imaginary part: stored as [real of all | imag of all]
        rows = torch.cat([torch.arange(0, 2 * cf, 2), torch.arange(1, 2 * cf, 2)]).to(device)
        blk['fdc'] = ops.ConvWeights.from_oihw(sd[f'{fu}.fdc.weight'][rows], sd[f'{fu}.fdc.bias'][rows], 3, fmt=PF_BF16, device=device)
        W[b] = blk

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
        W: dict = {'conv0': cw(sd['in_to_dim.weight'], sd['in_to_dim.bias'])}
        for i in range(self.n_block):
            self._pack_block(W, sd, f'gfisr_body.{i}', products, device)
        t = self.n_block
        W['tail0'] = cw(sd[f'gfisr_body.{t}.weight'], sd[f'gfisr_body.{t}.bias'])
        W['tail1'] = cw(sd[f'gfisr_body.{t + 2}.weight'], sd[f'gfisr_body.{t + 2}.bias'])
        W['zeros'] = torch.zeros(self.dim, dtype=torch.float32, device=device)
        self._pack_head3(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def _pack_head3(self, W, sd, products, device) -> None:
        """UniUpsampleV3 under ``upscale`` into ``W`` (FIGSR's head too: it reads ``head``, ``scale``, ``layers``, ``dys_index``, ``dim``,
        ``mid_dim`` and ``out_ch`` of the module)."""
        head = sd
        dys3 = self.dys_index is not None and self.scale != 1
        if dys3:
            # a 3x3 end convolution runs AFTER the sampling, at output resolution: rsa_dysample samples the features themselves, 8 channels
            # per launch through a selection matrix, and the convolution reads them as planes (as SMoSR's d_kernel = 3 head)
            d = f'upscale.{self.dys_index}'
            mid = self.mid_dim if self.dys_index else self.dim
            W['dys.end3'] = ops.ConvWeights.from_oihw(sd[f'{d}.end_conv.weight'], sd[f'{d}.end_conv.bias'], products, device=device)
            sel = torch.eye(mid, dtype=torch.float32, device=device)
            W['dys.sel'] = [sel[8 * g : 8 * g + 8].contiguous() for g in range(mid // 8)]
            W['dys.zero'] = torch.zeros(8, dtype=torch.float32, device=device)
            head = dict(sd)
            head[f'{d}.end_conv.weight'], head[f'{d}.end_conv.bias'] = torch.zeros((8, mid, 1, 1), device=device), W['dys.zero']
        pack_head(W, head, 'upscale', self.head, self.scale, self.layers, self.dys_index, 8 if dys3 else self.out_ch, products, device)

    def macs_per_input_pixel(self) -> int:
        """Convolution and depthwise MACs per pixel; the dense DFT is not a per-pixel cost (O(H + W) per pixel) and is left out."""
        d, h, cf = self.dim, self.hidden, self.cf
        blk = 9 * d * 2 * h + (9 + 22) * self.gc + 9 * h * d + 2 * cf * 2 * cf + 9 * 2 * cf
        head = sum(co * ci * k * k for _, co, ci, k in self.layers)
        return 9 * self.in_ch * d + self.n_block * blk + 9 * d * 2 * d * 2 + head

    # ---------------------------------------------------------------- plan
    def _dft(self, plan: Plan, tabs, inverse: bool, n, H, Wd, spec, scratch, planes: Planes, plane0: int, post=None, eps: float = EPS) -> None:
        dp = LG.GfisrDftParams()
        dp.batch, dp.H, dp.W, dp.C, dp.inverse, dp.fmt, dp.eps = n, H, Wd, self.cf, int(inverse), planes.fmt, eps
        dp.tab_row = tabs['row_inv' if inverse else 'row_fwd'].data_ptr()
        dp.tab_col = tabs['col_inv' if inverse else 'col_fwd'].data_ptr()
        dp.spec, dp.scratch = spec.data_ptr(), scratch.data_ptr()
        if post is not None:
            dp.norm_scale, dp.norm_offset = post[0].data_ptr(), post[1].data_ptr()
        planes.bind(dp, 'plane', plane0)
        Wf = Wd // 2 + 1
        flop = 2 * (H * Wd * 2 * Wf + 4 * H * H * Wf) * self.cf * n  # the issue's model: the row pass and the complex column pass
        unit = 2 * (2 if planes.lo is not None else 1)
        nbytes = n * self.cf * (H * Wd * unit + 2 * H * Wf * 4)
        label = f'{"inverse + post_norm" if inverse else "forward"}, {H}x{Wd}, {self.cf} channels'
        plan.launch('rsa_gfisr_dft', dp, kernels=2, meta=dict(kernel='rsa_gfisr_dft', flop=flop, bytes=nbytes, label=label))

    def _emit_block(self, plan: Plan, blk, n, H, Wd, cur, bufs):
        N_pl, F_pl, M_pl, spec, SP, scratch, tabs = (bufs[k] for k in ('norm', 'fc1', 'gate', 'spec', 'sp', 'scratch', 'tabs'))
        sc, off = blk['norm']
        cf, Wf = self.cf, Wd // 2 + 1
        hp, i_pl, f_pl = blk['planes'], blk['i_planes'], blk['f_planes']
        plan.launch('rsa_rmsnorm', dict(x_f32=cur, batch=n, H=H, W=Wd, C=self.dim, eps=EPS, scale=sc, offset=off, out=N_pl))
        plan.conv(ops.conv_params(blk['fc1'], N_pl, H, Wd, out=F_pl))
        self._dft(plan, tabs, False, n, H, Wd, spec, scratch, F_pl, hp + i_pl)
        sp = LG.GfisrSpectralParams()
        sp.batch, sp.H, sp.W, sp.C, sp.eps = n, H, Wf, 2 * cf, EPS
        sp.x, sp.scale, sp.offset = spec.data_ptr(), blk['rn'][0].data_ptr(), blk['rn'][1].data_ptr()
        sp.weight, sp.bias = blk['fpe'][0].data_ptr(), blk['fpe'][1].data_ptr()
        SP.bind(sp, 'out')
        # byte model: the f32 map read once (the halo re-reads stay on chip), hi and lo planes written once
        plan.launch('rsa_gfisr_spectral', sp, meta=dict(kernel='rsa_gfisr_spectral', flop=0, bytes=n * H * Wf * (2 * cf * 4 + SP.planes * 32)))
        plan.conv(ops.conv_params(blk['fdc'], SP, H, Wf, act=L.ACT_GELU, out_f32=spec))
        self._dft(plan, tabs, True, n, H, Wd, spec, scratch, F_pl, hp + i_pl, post=blk['post'])
        gp = L.GatedDwConvParams()
        gp.batch, gp.H, gp.W, gp.fmt, gp.i_planes, gp.n_segments = n, H, Wd, F_pl.fmt, i_pl + f_pl, len(blk['segs'])
        for s, (pl, kh, kw, wt, bt) in enumerate(blk['segs']):
            gp.seg[s].planes, gp.seg[s].kh, gp.seg[s].kw = pl, kh, kw
            gp.seg[s].weight, gp.seg[s].bias = wt.data_ptr(), bt.data_ptr()
        F_pl.bind(gp, 'g')
        F_pl.bind(gp, 'x', hp)
        M_pl.bind(gp, 'out')
        unit = 16 * (2 if F_pl.lo is not None else 1)
        plan.launch('rsa_gfisr_gate', dict(p=gp, act=L.ACT_SILU), meta=dict(kernel='rsa_gfisr_gate', flop=0, bytes=n * H * Wd * unit * 3 * hp))
        return M_pl

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, H, Wd = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        if H * (Wd // 2 + 1) == 1:
            # the reference's view_as_complex raises on the 1 x 1 half spectrum: a [.., 1, 1, 2] tensor that counts as contiguous with strides
            # it rejects.  1 x 2, 2 x 1, 1 x 3 and 3 x 1 run (tests/golden/gfisrv2_tiny_probe.npz)
            raise RuntimeError('Tensor must have a stride divisible by 2 for all but last dimension (a 1 x 1 input: the reference raises in view_as_complex)')
        s, dim, cf = self.scale, self.dim, self.cf
        pd = dim // 8
        Wf = Wd // 2 + 1
        with_lo = products == 3
        dev = plan.device
        x_pl = plan.planes(n, 1, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)

        trunk, S0, S1, R = (plan.f32map(n, dim, H, Wd) for _ in range(4))  # in_to_dim's output (the trunk residual), the stream, fc2 + SiLU
        feat = plan.planes(n, pd, H, Wd, with_lo)
        hp = W['gfisr_body.0']['planes']
        nbytes = int(L.load().rsa_gfisr_dft_scratch_bytes(n, cf, H, Wd))
        if nbytes <= 0:
            raise RuntimeError(f'GFISRv2: a {H}x{Wd} map is too large for the dense DFT (rsa_gfisr_dft)')
        bufs = dict(norm=plan.planes(n, pd, H, Wd, with_lo, fmt=PF_BF16), fc1=plan.planes(n, 2 * hp, H, Wd, with_lo), gate=plan.planes(n, hp, H, Wd, with_lo),
                    spec=plan.f32map(n, 2 * cf, H, Wf), sp=plan.planes(n, (2 * cf + 7) // 8, H, Wf, True, fmt=PF_BF16),
                    scratch=torch.empty(nbytes // 4, dtype=torch.float32, device=dev), tabs=LG.dft_tables(H, Wd, dev))  # fmt: skip
        plan.keep += [bufs['scratch'], *bufs['tabs'].values()]
        stats = self._unit_stats(n, dev)
        plan.keep.append(stats)
        plan.conv(ops.conv_params(W['conv0'], x_pl, H, Wd, out_f32=trunk))
        cur, nxt = trunk, S0
        for i in range(self.n_block):
            blk = W[f'gfisr_body.{i}']
            m = self._emit_block(plan, blk, n, H, Wd, cur, bufs)
            last = i == self.n_block - 1
            plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, act=L.ACT_SILU, out_f32=R))
            ap = plk.group_norm_apply_params(R, dim, 1, stats, blk['gamma'], W['zeros'], cur, feat if last else None, None if last else nxt)
            plan.launch('rsa_group_norm_apply', ap)
            cur, nxt = nxt, (S1 if nxt is S0 else S0)
        t1 = plan.planes(n, 2 * pd, H, Wd, with_lo)
        fe = plan.planes(n, pd, H, Wd, with_lo)
        dys3 = self.dys_index is not None and s != 1
        fe32 = plan.f32map(n, dim, H, Wd) if dys3 and self.dys_index == 0 else None
        plan.conv(ops.conv_params(W['tail0'], feat, H, Wd, act=L.ACT_SILU, out=t1))
        plan.conv(ops.conv_params(W['tail1'], t1, H, Wd, res1=trunk, alpha=1.0, out=fe, out_f32=fe32))
        # (the reference crops to 4 H x 4 W whatever the scale: nothing for scales up to 4)
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype)
        if dys3:
            self._emit_dys3(plan, W, fe, fe32, y, n, H, Wd, with_lo)
        else:
            emit_head(plan, W, self.head, s, self.layers, dim, self.mid_dim, self.dys_index, fe, None, y, n, H, Wd, with_lo)
        return set_input

    def _emit_dys3(self, plan: Plan, W, fe, fe32, y, n, H, Wd, with_lo) -> None:
        """DySample with its 3x3 end convolution: (mid_dim conv + LeakyReLU 0.01,) the offsets, then the sampled FEATURES at output
        resolution (rsa_dysample, 8 channels per launch through a selection matrix) as planes, and the end convolution on them."""
        s = self.scale
        x, x32, mid = fe, fe32, self.dim
        if self.dys_index == 2:
            mid = self.mid_dim
            x = plan.planes(n, mid // 8, H, Wd, with_lo)
            x32 = plan.f32map(n, mid, H, Wd)
            plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.01, out=x, out_f32=x32))
        offscope = plan.f32map(n, 4 * GROUPS * s * s, H, Wd)
        plan.conv(ops.conv_params(W['dys.offscope'], x, H, Wd, out_f32=offscope))
        up = plan.planes(n, mid // 8, s * H, s * Wd, with_lo)
        d = W['dys']
        for g, sel in enumerate(W['dys.sel']):
            t = torch.empty((n, 8, s * H, s * Wd), dtype=torch.float32, device=plan.device)
            plan.keep.append(t)
            dp = L.DySampleParams()
            dp.batch, dp.H, dp.W, dp.C, dp.groups, dp.scale, dp.out_ch = n, H, Wd, mid, GROUPS, s, 8
            dp.x_f32, dp.offscope = x32.data_ptr(), offscope.data_ptr()
            dp.init_pos, dp.end_b, dp.end_w = d['init_pos'].data_ptr(), W['dys.zero'].data_ptr(), sel.data_ptr()
            dp.out_nchw, dp.out_dtype = t.data_ptr(), L.F32
            plan.launch('rsa_dysample', dp)
            one = Planes(up.hi[:, g : g + 1], None if up.lo is None else up.lo[:, g : g + 1])
            plan.call(lambda src=t, dst=one: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
        plan.conv(ops.conv_params(W['dys.end3'], up, s * H, s * Wd, out_nchw=y))
