"""LAWFFT on the MI355X engine (reference module: ``resselt/archs/lawfft/arch.py:380-434``), eval-mode semantics.

Trunk: reflect pad on the bottom and right to a multiple of 8 (in the conversion of the caller's tensor into planes), in_to_dim 3x3,
``n_rblock`` ResidualMeta (``n_mblock`` MetaBlocks, a DynamicLocal(dim, 3) and the group's residual), ``+ in_to_dim's output``, then
UniUpsample (version 2) through ``engine/uniupsample.py``, cropped to ``h scale x w scale``.

A MetaBlock is ``x += SFSAS(LN(x)); x += FeedForward(LN(x))`` on an f32 residual stream.  At pack time

  * ``to_hidden``'s columns are zero-embedded over all ``dim`` channels of ``LN(x)`` (the channel split costs nothing) and its rows, like
    ``to_hidden_dw``'s, are laid out as [q | k | v], each padded to whole planes;
  * ``project_out`` is folded into ``last`` in float64: ``last(cat[x1, P z + b]) = L1 x1 + (L2 P) z + (L2 b + b_last)``, one 1x1 over the
    planes [x1 | z] with the block's residual in its epilogue;
  * FeedForward's ``project_in`` / ``dwconv`` rows are laid out as [x1 | x2], each padded to whole planes (``rsa_eimn_sal`` is its middle).

Launch steps per MetaBlock, windowed (odd blocks): rsa_layernorm, 2 x (rsa_lawfft_kernel_gen [pool + generate], rsa_lawfft_dyn_dwconv),
to_hidden 1x1, rsa_dwconv3x3, rsa_lawfft_wincorr, last 1x1, rsa_layernorm, project_in 1x1, rsa_eimn_sal, project_out 1x1 = 13 steps, 15
kernels.  Whole-image (even blocks): rsa_lawfft_wincorr is replaced by rsa_gfisr_dft (q), rsa_gfisr_dft (k), rsa_lawfft_spec_mul,
rsa_gfisr_dft (inverse, no norm) and rsa_lawfft_norm_mul = 17 steps, 22 kernels.  The DFT tables are the 'ortho' ones of
``lib_gfisr.dft_tables``: torch's default 'backward' normalisation of ``irfft2(rfft2(q) rfft2(k))`` is ``sqrt(H W)`` times the ortho
chain, which is ``rsa_lawfft_spec_mul``'s ``scale``.  Spectral values stay f32 and the correlation is written as bf16 split planes (hi +
lo: f32 range) in every precision policy.  Nothing is read back to the host: the pooled means, the generated kernels and the spectra
live in plan buffers.
"""

from __future__ import annotations

import math

import torch

from ...engine import lib as L
from ...engine import lib_lawfft as LW
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.fourier import dft_workspace, emit_dft
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ...engine.uniupsample import SAMPLE_MODS, Head, OwnMetaUpsample

MAX_DIM = 128  # the LAWFFT kernels and rsa_gfisr_dft: at most 128 channels
EPS = 1e-6
WINDOW = 8


def _planes(c: int) -> int:
    return (c + 7) // 8


def _padded(t: torch.Tensor, rows: int) -> torch.Tensor:
    out = torch.zeros((rows, *t.shape[1:]), dtype=torch.float32, device=t.device)
    out[: t.shape[0]] = t
    return out.contiguous()


def _chunked(t: torch.Tensor, chunks: int, width: int) -> torch.Tensor:
    """Rows [chunk 0 | chunk 1 | ...] of ``width`` each -> the same chunks, each from a plane boundary (zero rows between them)."""
    pw = 8 * _planes(width)
    out = torch.zeros((chunks * pw, *t.shape[1:]), dtype=t.dtype, device=t.device)
    for c in range(chunks):
        out[c * pw : c * pw + width] = t[c * width : (c + 1) * width]
    return out


class LAWFFT(OwnMetaUpsample, EngineModule):  # (the reference's load_state_dict override: arch.py:418-420)
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'fp16')
    global_statistics = True  # DynamicLocal's pooling and the whole-image correlation span the tensor they are given

    def __init__(self, in_ch: int = 3, dim: int = 60, split: float = 0.25, scale: int = 4, n_rblock: int = 4, n_mblock: int = 6,
                 t_mid_factor: float = 1.0, window_size: int = 8, mlp_factor: float = 2.66, unshuffle_mod: bool = False,
                 upsampler: str = 'pixelshuffledirect', mid_dim: int = 48, local: int | None = None, fsas: int | None = None,
                 hidden: int | None = None, to_hidden_rows: int | None = None) -> None:  # fmt: skip
        """``local``, ``fsas`` (the width of q, k and v), ``hidden`` (FeedForward's) and ``to_hidden_rows``: what a checkpoint's shapes give
        (the loader reads them); otherwise ``int(split dim)``, ``int(global t_mid_factor)``, ``int(dim mlp_factor)`` and
        ``int(global 3 t_mid_factor)`` as the reference computes them."""
        super().__init__()
        if window_size != WINDOW:
            raise NotImplementedError(f'LAWFFT: window_size {window_size} is not built (8 is)')
        if unshuffle_mod:
            raise NotImplementedError('LAWFFT: unshuffle_mod checkpoints (in_to_dim.1.weight) are not built (the reference does not load them either: '
                                      'its loader does not detect a checkpoint without in_to_dim.weight)')  # fmt: skip
        if dim < 2 or dim > MAX_DIM:
            raise NotImplementedError(f'LAWFFT: dim must be in 2..{MAX_DIM} (got {dim})')
        if in_ch < 1 or in_ch > 8:
            raise NotImplementedError(f'LAWFFT: 1 to 8 input channels are built (got {in_ch})')
        local = int(split * dim) if local is None else int(local)
        glob = dim - local
        if local < 1 or glob < 1:
            raise NotImplementedError(f'LAWFFT: the local and the global width must be at least 1 (got {local} and {glob} of dim {dim})')
        fsas = int(glob * t_mid_factor) if fsas is None else int(fsas)
        rows = int(glob * 3 * t_mid_factor) if to_hidden_rows is None else int(to_hidden_rows)
        if fsas < 1 or fsas > MAX_DIM:
            raise NotImplementedError(f'LAWFFT: the FSAS width int(global * t_mid_factor) must be in 1..{MAX_DIM} (got {fsas})')
        if rows != 3 * fsas:
            raise NotImplementedError(f'LAWFFT: to_hidden must have 3 x the FSAS width rows (got {rows} for a width of {fsas}: q, k and v would not be equal chunks)')
        hidden = int(dim * mlp_factor) if hidden is None else int(hidden)
        if hidden < 1:
            raise NotImplementedError(f'LAWFFT: the FeedForward width int(dim * mlp_factor) must be at least 1 (got {hidden})')
        if n_rblock < 1:
            raise NotImplementedError('LAWFFT: at least one ResidualMeta')
        if n_mblock < 2:
            raise NotImplementedError('LAWFFT: at least two MetaBlocks per ResidualMeta (the reference\'s loader reads block 1)')
        if upsampler not in SAMPLE_MODS:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')
        self.in_ch = self.out_ch = in_ch
        self.scale, self.dim, self.local, self.glob, self.fsas, self.hidden = scale, dim, local, glob, fsas, hidden
        self.n_rblock, self.n_mblock, self.head, self.mid_dim = n_rblock, n_mblock, upsampler, mid_dim
        self.up = Head('upscale', upsampler, scale, dim, in_ch, mid_dim)
        if scale != 1 and mid_dim % 8 and (upsampler == 'pixelshuffle' or self.up.dys_index == 2):
            raise NotImplementedError(f'LAWFFT: the {upsampler} head needs mid_dim to be a multiple of 8 (got {mid_dim})')
        shapes: dict = {'in_to_dim.weight': (dim, in_ch, 3, 3), 'in_to_dim.bias': (dim,)}

        def gen(name, c, k):
            shapes[f'{name}.kernel_gen.1.weight'], shapes[f'{name}.kernel_gen.1.bias'] = (c, c, 1, 1), (c,)
            shapes[f'{name}.kernel_gen.3.weight'], shapes[f'{name}.kernel_gen.3.bias'] = (c * k * k, c, 1, 1), (c * k * k,)

        for r in range(n_rblock):
            for i in range(n_mblock):
                b = f'body.{r}.residual.{i}'
                t, a, c = f'{b}.token_mix', f'{b}.token_mix.1.att', f'{b}.channel_mix1'
                shapes[f'{t}.0.weight'], shapes[f'{t}.0.bias'] = (dim,), (dim,)
                gen(f'{t}.1.local.0', local, 3)
                gen(f'{t}.1.local.1', local, 5)
                shapes[f'{a}.to_hidden.weight'], shapes[f'{a}.to_hidden.bias'] = (3 * fsas, glob, 1, 1), (3 * fsas,)
                shapes[f'{a}.to_hidden_dw.weight'], shapes[f'{a}.to_hidden_dw.bias'] = (3 * fsas, 1, 3, 3), (3 * fsas,)
                shapes[f'{a}.project_out.weight'], shapes[f'{a}.project_out.bias'] = (glob, fsas, 1, 1), (glob,)
                shapes[f'{a}.norm.weight'], shapes[f'{a}.norm.bias'] = (fsas,), (fsas,)
                shapes[f'{t}.1.last.weight'], shapes[f'{t}.1.last.bias'] = (dim, dim, 1, 1), (dim,)
                shapes[f'{c}.0.weight'], shapes[f'{c}.0.bias'] = (dim,), (dim,)
                shapes[f'{c}.1.project_in.weight'], shapes[f'{c}.1.project_in.bias'] = (2 * hidden, dim, 1, 1), (2 * hidden,)
                shapes[f'{c}.1.dwconv.weight'], shapes[f'{c}.1.dwconv.bias'] = (2 * hidden, 1, 3, 3), (2 * hidden,)
                shapes[f'{c}.1.project_out.weight'], shapes[f'{c}.1.project_out.bias'] = (dim, hidden, 1, 1), (dim,)
            gen(f'body.{r}.residual.{n_mblock}', dim, 3)
        buffers = {'window_size': torch.tensor(window_size, dtype=torch.uint8)}
        self.up.shapes(shapes, buffers)
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack_block(self, W, sd, b, products, device) -> None:
        dim, local, glob, cw, hid = self.dim, self.local, self.glob, self.fsas, self.hidden
        P_l, P_w = _planes(local), _planes(cw)
        d, f32 = torch.float64, torch.float32
        cv = lambda w, bias: ops.ConvWeights.from_oihw(w.to(f32)[:, :, None, None], bias.to(f32), products, device=device)  # noqa: E731
        t, a, c = f'{b}.token_mix', f'{b}.token_mix.1.att', f'{b}.channel_mix1'
        blk = {'ln1': (sd[f'{t}.0.weight'].contiguous(), sd[f'{t}.0.bias'].contiguous())}
        for j in range(2):
            g = f'{t}.1.local.{j}.kernel_gen'
            blk[f'gen{j}'] = LW.pack_kernel_gen(sd[f'{g}.1.weight'], sd[f'{g}.1.bias'], sd[f'{g}.3.weight'], sd[f'{g}.3.bias'])
        # to_hidden reads all dim channels of LN(x): zero columns for the local ones; rows [q | k | v] from plane boundaries
        th = torch.zeros((3 * cw, dim), dtype=f32, device=device)
        th[:, local:] = sd[f'{a}.to_hidden.weight'].reshape(3 * cw, glob)
        blk['to_hidden'] = cv(_chunked(th, 3, cw), _chunked(sd[f'{a}.to_hidden.bias'], 3, cw))
        blk['dw'] = (_chunked(sd[f'{a}.to_hidden_dw.weight'].reshape(3 * cw, 9), 3, cw).contiguous(), _chunked(sd[f'{a}.to_hidden_dw.bias'], 3, cw).contiguous())
        blk['att_norm'] = (_padded(sd[f'{a}.norm.weight'], 8 * P_w), _padded(sd[f'{a}.norm.bias'], 8 * P_w))
        # last(cat[x1, P z + b]) = L1 x1 + (L2 P) z + (L2 b + b_last), in float64
        lw, lb = sd[f'{t}.1.last.weight'].reshape(dim, dim).to(d), sd[f'{t}.1.last.bias'].to(d)
        pw, pb = sd[f'{a}.project_out.weight'].reshape(glob, cw).to(d), sd[f'{a}.project_out.bias'].to(d)
        w = torch.zeros((dim, 8 * (P_l + P_w)), dtype=d, device=device)
        w[:, :local] = lw[:, :local]
        w[:, 8 * P_l : 8 * P_l + cw] = lw[:, local:] @ pw
        blk['last'] = cv(w, lw[:, local:] @ pb + lb)
        blk['ln2'] = (sd[f'{c}.0.weight'].contiguous(), sd[f'{c}.0.bias'].contiguous())
        blk['pin'] = cv(_chunked(sd[f'{c}.1.project_in.weight'].reshape(2 * hid, dim), 2, hid), _chunked(sd[f'{c}.1.project_in.bias'], 2, hid))
        blk['sal'] = (_chunked(sd[f'{c}.1.dwconv.weight'].reshape(2 * hid, 9), 2, hid).contiguous(), _chunked(sd[f'{c}.1.dwconv.bias'], 2, hid).contiguous())
        blk['pout'] = cv(sd[f'{c}.1.project_out.weight'].reshape(dim, hid), sd[f'{c}.1.project_out.bias'])
        W[b] = blk

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if k not in ('window_size', 'upscale.MetaUpsample')}
        W: dict = {'conv0': ops.ConvWeights.from_oihw(sd['in_to_dim.weight'], sd['in_to_dim.bias'], products, device=device)}
        for r in range(self.n_rblock):
            for i in range(self.n_mblock):
                self._pack_block(W, sd, f'body.{r}.residual.{i}', products, device)
            g = f'body.{r}.residual.{self.n_mblock}.kernel_gen'
            W[f'body.{r}.gen'] = LW.pack_kernel_gen(sd[f'{g}.1.weight'], sd[f'{g}.1.bias'], sd[f'{g}.3.weight'], sd[f'{g}.3.bias'])
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            convs = [v for v in W.values() if isinstance(v, ops.ConvWeights)]
            convs += [v for blk in W.values() if isinstance(blk, dict) for v in blk.values() if isinstance(v, ops.ConvWeights)]
            check_fp16_range(convs)
        return W

    def macs_per_input_pixel(self) -> int:
        """Convolution, depthwise and windowed-correlation MACs per pixel of the padded map; the dense DFT of the whole-image blocks is not
        a per-pixel cost (O(H + W) per pixel) and is left out."""
        d, lo, cw, hid = self.dim, self.local, self.fsas, self.hidden
        blk = d * 3 * cw + 27 * cw + (9 + 25) * lo + (lo + cw) * d + d * 2 * hid + 18 * hid + hid * d
        win = (self.n_mblock // 2) * 64 * cw
        return 9 * self.in_ch * d + self.n_rblock * (self.n_mblock * blk + win + 9 * d) + self.up.macs()

    # ---------------------------------------------------------------- plan
    def _dynamic_local(self, plan: Plan, gen, k, C, src: Planes, src_plane0, bufs, n, H, Wd, out: Planes | None = None, out_plane0: int = 0, res1=None,
                       res2=None, out_f32=None) -> None:  # fmt: skip
        """DynamicLocal(C, k) on the planes ``src`` from ``src_plane0``: the generator (pool, two linear layers) into the plan's kernel
        buffer, then the per-sample depthwise convolution."""
        w1_t, b1, w2_t, b2 = gen
        unit = 16 * (2 if src.lo is not None else 1)
        px = n * H * Wd
        gp = LW.LawfftKernelGenParams()
        gp.batch, gp.H, gp.W, gp.C, gp.ksize, gp.fmt = n, H, Wd, C, k, src.fmt
        gp.w1_t, gp.b1, gp.w2_t, gp.b2 = w1_t.data_ptr(), b1.data_ptr(), w2_t.data_ptr(), b2.data_ptr()
        gp.workspace, gp.out = bufs['gen_ws'].data_ptr(), bufs['kernels'].data_ptr()
        src.bind(gp, 'in', src_plane0)
        plan.launch('rsa_lawfft_kernel_gen', gp, kernels=2, meta=dict(kernel='rsa_lawfft_kernel_gen', flop=0, bytes=px * _planes(C) * unit))
        dp = LW.LawfftDynDwConvParams()
        dp.batch, dp.H, dp.W, dp.C, dp.ksize, dp.fmt = n, H, Wd, C, k, src.fmt
        dp.weight = bufs['kernels'].data_ptr()
        dp.res1, dp.res2 = (None if r is None else r.data_ptr() for r in (res1, res2))
        dp.out_f32 = None if out_f32 is None else out_f32.data_ptr()
        src.bind(dp, 'in', src_plane0)
        if out is not None:
            out.bind(dp, 'out', out_plane0)
        maps = sum(1 for m in (res1, res2, out_f32) if m is not None)
        nbytes = px * (_planes(C) * unit * (2 if out is not None else 1) + maps * 4 * ((C + 3) // 4) * 4)
        plan.launch('rsa_lawfft_dyn_dwconv', dp, meta=dict(kernel='rsa_lawfft_dyn_dwconv', flop=2 * px * C * k * k, bytes=nbytes))

    def _layernorm(self, plan: Plan, gb, x_f32, out: Planes, n, H, Wd) -> None:
        lp = L.LayerNormParams()
        lp.batch, lp.H, lp.W, lp.C, lp.eps = n, H, Wd, self.dim, EPS
        lp.x_f32, lp.gamma, lp.beta = x_f32.data_ptr(), gb[0].data_ptr(), gb[1].data_ptr()
        out.bind(lp, 'out')
        lp.out_fmt = out.fmt
        plan.launch('rsa_layernorm', lp)

    def _emit_fsas(self, plan: Plan, blk, windowed: bool, bufs, n, H, Wd) -> None:
        """q, k, v = the three plane ranges of D; out = v * LN(corr) into the planes of CAT behind the local ones."""
        D, CAT = bufs['dw'], bufs['cat']
        cw, P_w, P_l = self.fsas, _planes(self.fsas), _planes(self.local)
        unit = 16 * (2 if D.lo is not None else 1)
        px = n * H * Wd
        gamma, beta = blk['att_norm']
        if windowed:
            wp = LW.LawfftWincorrParams()
            wp.batch, wp.H, wp.W, wp.C, wp.fmt, wp.eps = n, H, Wd, cw, D.fmt, EPS
            wp.weight, wp.bias = gamma.data_ptr(), beta.data_ptr()
            D.bind(wp, 'q')
            D.bind(wp, 'k', P_w)
            D.bind(wp, 'v', 2 * P_w)
            CAT.bind(wp, 'out', P_l)
            # byte model: q, k and v read once, the output written once
            plan.launch('rsa_lawfft_wincorr', wp, meta=dict(kernel='rsa_lawfft_wincorr', flop=2 * 64 * px * cw, bytes=px * 4 * P_w * unit))
            return
        A, B, CORR = bufs['spec_a'], bufs['spec_b'], bufs['corr']
        Wf = Wd // 2 + 1
        emit_dft(plan, bufs['dft'], False, n, cw, H, Wd, A, D, 0)
        emit_dft(plan, bufs['dft'], False, n, cw, H, Wd, B, D, P_w)
        sp = LW.LawfftSpecMulParams()
        sp.batch, sp.H, sp.W, sp.C, sp.scale = n, H, Wf, cw, math.sqrt(H * Wd)
        sp.a, sp.b, sp.out = A.data_ptr(), B.data_ptr(), A.data_ptr()
        plan.launch('rsa_lawfft_spec_mul', sp, meta=dict(kernel='rsa_lawfft_spec_mul', flop=8 * n * H * Wf * cw, bytes=3 * n * H * Wf * 2 * cw * 4))
        emit_dft(plan, bufs['dft'], True, n, cw, H, Wd, A, CORR, 0)
        nm = LW.LawfftNormMulParams()
        nm.batch, nm.H, nm.W, nm.C, nm.corr_fmt, nm.fmt, nm.eps = n, H, Wd, cw, CORR.fmt, D.fmt, EPS
        nm.weight, nm.bias = gamma.data_ptr(), beta.data_ptr()
        CORR.bind(nm, 'corr')
        D.bind(nm, 'v', 2 * P_w)
        CAT.bind(nm, 'out', P_l)
        plan.launch('rsa_lawfft_norm_mul', nm, meta=dict(kernel='rsa_lawfft_norm_mul', flop=0, bytes=px * P_w * (32 + 2 * unit)))

    def _emit_block(self, plan: Plan, blk, windowed: bool, bufs, n, H, Wd, cur, mid, nxt, x_planes: Planes | None) -> None:
        """One MetaBlock: ``cur`` -> token mix -> ``mid`` -> channel mix -> ``nxt`` (f32 maps; ``x_planes``: the result as planes too)."""
        N, T, D, LOC, CAT, S, G = (bufs[k] for k in ('norm', 'hidden', 'dw', 'local', 'cat', 'pin', 'gate'))
        P_w, P_h = _planes(self.fsas), _planes(self.hidden)
        unit = 16 * (2 if N.lo is not None else 1)
        px = n * H * Wd
        self._layernorm(plan, blk['ln1'], cur, N, n, H, Wd)
        # the local branch: the first planes of LN(x), whose channels past `local` belong to the global branch and are masked by C
        self._dynamic_local(plan, blk['gen0'], 3, self.local, N, 0, bufs, n, H, Wd, out=LOC)
        self._dynamic_local(plan, blk['gen1'], 5, self.local, LOC, 0, bufs, n, H, Wd, out=CAT)
        plan.conv(ops.conv_params(blk['to_hidden'], N, H, Wd, out=T))
        dp = L.DwConvParams()
        dp.batch, dp.H, dp.W, dp.planes, dp.act, dp.fmt = n, H, Wd, 3 * P_w, L.ACT_NONE, T.fmt
        T.bind(dp, 'in')
        dp.weight, dp.bias = blk['dw'][0].data_ptr(), blk['dw'][1].data_ptr()
        D.bind(dp, 'out')
        plan.launch('rsa_dwconv3x3', dp, meta=dict(kernel='rsa_dwconv3x3', flop=2 * px * 9 * 3 * self.fsas, bytes=px * 6 * P_w * unit))
        self._emit_fsas(plan, blk, windowed, bufs, n, H, Wd)
        plan.conv(ops.conv_params(blk['last'], CAT, H, Wd, res1=cur, alpha=1.0, out_f32=mid))
        self._layernorm(plan, blk['ln2'], mid, N, n, H, Wd)
        plan.conv(ops.conv_params(blk['pin'], N, H, Wd, out=S))
        plan.launch('rsa_eimn_sal', dict(in_=S, out=G, batch=n, H=H, W=Wd, planes=P_h, fmt=S.fmt, weight=blk['sal'][0], bias=blk['sal'][1]),
                    meta=dict(kernel='rsa_eimn_sal', flop=2 * px * 16 * P_h * 9, bytes=px * P_h * unit * 3))  # fmt: skip
        plan.conv(ops.conv_params(blk['pout'], G, H, Wd, res1=mid, alpha=1.0, out_f32=nxt, out=x_planes))

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        ph, pw_ = (WINDOW - h0 % WINDOW) % WINDOW, (WINDOW - w0 % WINDOW) % WINDOW
        if ph >= h0 or pw_ >= w0:
            # the reference's F.pad raises: a reflection of p pixels needs more than p of them (sides 1 to 4 raise, 5 to 8 run)
            raise RuntimeError(f'Padding size should be less than the corresponding input dimension (a {h0}x{w0} input: LAWFFT pads by ({ph}, {pw_}))')
        s, dim, cw = self.scale, self.dim, self.fsas
        H, Wd = h0 + ph, w0 + pw_
        Wf = Wd // 2 + 1
        pd, P_l, P_w, P_h = _planes(dim), _planes(self.local), _planes(cw), _planes(self.hidden)
        with_lo = products == 3
        dev = plan.device
        x_pl = plan.planes(n, 1, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)  # the reflect pad on the bottom and right happens in the conversion

        dft = dft_workspace(plan, 'LAWFFT', n, cw, H, Wd)
        ws_bytes = int(L.load().rsa_lawfft_kernel_gen_workspace_bytes(n, dim, H, Wd))
        f32 = torch.float32
        bufs = dict(norm=plan.planes(n, pd, H, Wd, with_lo), hidden=plan.planes(n, 3 * P_w, H, Wd, with_lo), dw=plan.planes(n, 3 * P_w, H, Wd, with_lo),
                    local=plan.planes(n, P_l, H, Wd, with_lo), cat=plan.planes(n, P_l + P_w, H, Wd, with_lo), pin=plan.planes(n, 2 * P_h, H, Wd, with_lo),
                    gate=plan.planes(n, P_h, H, Wd, with_lo), spec_a=plan.f32map(n, 2 * cw, H, Wf), spec_b=plan.f32map(n, 2 * cw, H, Wf),
                    corr=plan.planes(n, P_w, H, Wd, True, fmt=PF_BF16), dft=dft, gen_ws=torch.empty(ws_bytes // 4, dtype=f32, device=dev),
                    kernels=torch.empty(n * 8 * pd * 25, dtype=f32, device=dev))  # fmt: skip
        plan.keep += [bufs['gen_ws'], bufs['kernels']]
        trunk, S0, S1, RB0, RB1 = (plan.f32map(n, dim, H, Wd) for _ in range(5))  # in_to_dim's output, the blocks' stream, the groups' inputs
        X = plan.planes(n, pd, H, Wd, with_lo)  # the last block's result as planes: what a group's DynamicLocal reads
        fe = plan.planes(n, pd, H, Wd, with_lo)
        fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None
        plan.conv(ops.conv_params(W['conv0'], x_pl, H, Wd, out_f32=trunk))
        rin = trunk
        for r in range(self.n_rblock):
            cur = rin
            for i in range(self.n_mblock):
                last = i == self.n_mblock - 1
                self._emit_block(plan, W[f'body.{r}.residual.{i}'], bool(i % 2), bufs, n, H, Wd, cur, S0, S1, X if last else None)
                cur = S1
            gen = W[f'body.{r}.gen']
            if r == self.n_rblock - 1:  # + the group's input + in_to_dim's output; the head reads planes (and DySample the f32 features)
                self._dynamic_local(plan, gen, 3, dim, X, 0, bufs, n, H, Wd, out=fe, res1=rin, res2=trunk, out_f32=fe32)
            else:
                rout = RB1 if rin is not RB1 else RB0
                self._dynamic_local(plan, gen, 3, dim, X, 0, bufs, n, H, Wd, res1=rin, out_f32=rout)
                rin = rout
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        self.up.emit(plan, W, fe, fe32, y, with_lo)
        return set_input
