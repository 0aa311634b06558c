"""PLKSR and RealPLKSR on the MI355X engine (reference modules: ``resselt/archs/plksr/plksr.py:259-323`` and ``rplksr.py:108-172``).

A block is  x -> channel mixer (two fused convolutions) -> partial large-kernel conv of the first pdim channels -> EA -> refine 1x1
-> (+ x for PLKSR | GroupNorm(4) + x for RealPLKSR).  Per block:
  * the mixer's second convolution is split by output channel at pack time: channels [0, pdim) go to a scratch buffer that rsa_plk_conv
    reads, channels [pdim, dim) straight to their planes of the block buffer -- the reference's in-place ``x[:, :pdim] = conv(...)``
    without a copy;
  * rsa_plk_conv writes planes [0, pdim/8) of the same buffer (the sparse large-kernel variants of PLKSR are folded into one dense K x K
    kernel at pack time, engine/plk.py);
  * EA: its 3x3 convolution writes an f32 map, rsa_ea_gate multiplies the block buffer by its sigmoid in place;
  * refine: a 1x1 convolution with the f32 skip as residual (PLKSR), or into an f32 map that rsa_group_norm_stats / _apply normalise
    over the whole image and add the skip to (RealPLKSR).
Head: ``feats[-1](x) + repeat_interleave(x, s^2)`` then PixelShuffle -- the final store adds the nearest-upsampled input (as Compact) --
or DySample: the image occupies the plane behind the features and the last convolution maps it with 0/1 weights (the repeat is a 1x1
convolution), so the DySample input exists as split planes; offset/scope and the pre-projected end convolution follow (as SPANPlus).
"""

from __future__ import annotations

import torch

from ...engine import dysample as dys
from ...engine import lib as L
from ...engine import ops, plk
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import Planes

_CCM_K = {'CCM': (3, 1), 'ICCM': (1, 3), 'DCCM': (3, 3)}  # kernel sizes of channel_mixer.0 / .2
_SPARSE = ((5, 1), (5, 2), (5, 3), (5, 4))  # the reference loader's fixed SparsePLK sub-kernels (archs/plksr/__init__.py: sparse_kernels / dilations)
NORM_GROUPS = 4


def _check_geometry(dim: int, pdim: int, kernel_size: int, in_ch: int) -> None:
    if in_ch != 3:
        raise NotImplementedError(f'PLKSR: only 3 input channels are built (got {in_ch})')
    if dim % 8:
        raise NotImplementedError(f'PLKSR: dim must be a multiple of 8 (got {dim})')
    if pdim % 8 or pdim < 8 or pdim > min(dim, 64):
        raise NotImplementedError(f'PLKSR: pdim = int(dim * split_ratio) must be a multiple of 8 in [8, min(dim, 64)] (got {pdim})')
    if kernel_size % 2 == 0 or kernel_size < 3 or kernel_size > 31:
        raise NotImplementedError(f'PLKSR: kernel_size must be odd and in [3, 31] (got {kernel_size})')


class _PLKBase(EngineModule):
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'fp16')
    _mixer_key = 'channel_mixer'
    _mixer_act = L.ACT_MISH
    _norm = False

    def _lk_weights(self, sd, b: int):
        raise NotImplementedError

    def _last_index(self) -> int:
        raise NotImplementedError

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        dim, pdim, s = self.dim, self.pdim, self.upscale
        W: dict = {'feats.0': ops.ConvWeights.from_oihw(sd['feats.0.weight'], sd['feats.0.bias'], products, device=device)}
        lk_raw = []
        for b in range(1, self.n_blocks + 1):
            p = f'feats.{b}'
            m = f'{p}.{self._mixer_key}'
            W[f'{p}.mix0'] = ops.ConvWeights.from_oihw(sd[f'{m}.0.weight'], sd[f'{m}.0.bias'], products, device=device)
            w2, b2 = sd[f'{m}.2.weight'], sd[f'{m}.2.bias']
            W[f'{p}.mix2a'] = ops.ConvWeights.from_oihw(w2[:pdim], b2[:pdim], products, device=device)
            if pdim < dim:
                W[f'{p}.mix2b'] = ops.ConvWeights.from_oihw(w2[pdim:], b2[pdim:], products, device=device)
            lk_w, lk_b = self._lk_weights(sd, b)
            lk_raw.append(lk_w)
            W[f'{p}.lk'] = (plk.pack_plk_weights(lk_w, int(products), products.fmt), plk.plk_bias(lk_b))
            if self.use_ea:
                W[f'{p}.ea'] = ops.ConvWeights.from_oihw(sd[f'{p}.attn.f.0.weight'], sd[f'{p}.attn.f.0.bias'], products, device=device)
            W[f'{p}.refine'] = ops.ConvWeights.from_oihw(sd[f'{p}.refine.weight'], sd[f'{p}.refine.bias'], products, device=device)
            if self._norm:
                W[f'{p}.norm'] = (sd[f'{p}.norm.weight'].contiguous(), sd[f'{p}.norm.bias'].contiguous())
        last = f'feats.{self._last_index()}'
        wl, bl = sd[f'{last}.weight'], sd[f'{last}.bias']
        if getattr(self, 'dysample', False):
            # [features | image plane] -> 3 s^2 channels: the image part is repeat_interleave(x, s^2) as 0/1 centre taps
            cin = dim + self.in_ch
            w = torch.zeros((wl.shape[0], cin, 3, 3), dtype=torch.float32, device=device)
            w[:, :dim] = wl
            for c in range(self.in_ch):
                w[c * s * s : (c + 1) * s * s, dim + c, 1, 1] = 1.0
            W['last'] = ops.ConvWeights.from_oihw(w, bl, products, cin_planes=dim // 8 + 1, device=device)
            self._pack_dysample(W, sd, device, products)
        else:
            W['last'] = ops.ConvWeights.from_oihw(wl, bl, products, device=device)
        if products.fmt == ops.PF_F16:
            check_fp16_range(W.values())
            if float(torch.stack([w.abs().amax() for w in lk_raw]).amax()) > 6.0e4:
                from ...engine.base import Fp16Range

                raise Fp16Range('a PLK weight exceeds the fp16 range (|w| > 6e4)')
        return W

    def _pack_dysample(self, W, sd, device, products):
        s, cin = self.upscale, self.in_ch * self.upscale**2
        if s != 1:
            end_w, end_b = sd['to_img.end_conv.weight'].reshape(self.in_ch, cin), sd['to_img.end_conv.bias']
        else:  # no end convolution (end_convolution = s != 1): the sampled channels are the output
            end_w, end_b = torch.eye(cin, device=device), torch.zeros(cin, device=device)
        dys.pack(W, sd['to_img.offset.weight'], sd['to_img.offset.bias'], sd['to_img.scope.weight'], end_w, end_b, sd['to_img.init_pos'],
                      self.dys_groups, s, products=products, device=device)  # fmt: skip

    def macs_per_input_pixel(self) -> int:
        d, p, s = self.dim, self.pdim, self.upscale
        k0, k2 = _CCM_K[self.ccm_type]
        blk = 2 * d * d * (k0 * k0 + k2 * k2) + p * p * self.kernel_size**2 + (9 * d * d if self.use_ea else 0) + d * d
        return 27 * d + self.n_blocks * blk + 9 * d * self.in_ch * s * s

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h, w = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        dim, pdim, s, nb = self.dim, self.pdim, self.upscale, self.n_blocks
        pf, pp = dim // 8, pdim // 8
        with_lo = products == 3
        dev = plan.device
        # block buffers: feature planes + one plane for the image (read by feats.0, and by the DySample head's last convolution)
        X = [plan.planes(n, pf + 1, h, w, with_lo) for _ in range(2)]
        Xf = [plan.f32map(n, dim, h, w) for _ in range(2)]
        T = plan.planes(n, 2 * pf, h, w, with_lo)
        Sb = plan.planes(n, pp, h, w, with_lo)
        M = plan.planes(n, pf, h, w, with_lo)
        G = plan.f32map(n, dim, h, w) if self.use_ea else None
        if self._norm:
            R = plan.f32map(n, dim, h, w)
            stats = torch.empty((n, NORM_GROUPS, 2), dtype=torch.float32, device=dev)
            ws = plk.group_norm_workspace(n, h, w, NORM_GROUPS, dev)
            plan.keep += [stats, ws]
        fin = X[nb % 2]
        img = Planes(fin.hi[:, pf : pf + 1], None if fin.lo is None else fin.lo[:, pf : pf + 1])

        def set_input(x):
            ops.nchw_to_planes(x, img)

        plan.conv(ops.conv_params(W['feats.0'], fin, h, w, in_plane0=pf, out=X[0], out_f32=Xf[0]))
        k0, _ = _CCM_K[self.ccm_type]
        for b in range(1, nb + 1):
            p = f'feats.{b}'
            xi, xo = (b - 1) % 2, b % 2
            plan.conv(ops.conv_params(W[f'{p}.mix0'], X[xi], h, w, act=self._mixer_act, out=T))
            plan.conv(ops.conv_params(W[f'{p}.mix2a'], T, h, w, out=Sb))
            if pdim < dim:
                plan.conv(ops.conv_params(W[f'{p}.mix2b'], T, h, w, out=M, out_plane_off=pp))
            blob, lk_bias = W[f'{p}.lk']
            plan.launch('rsa_plk_conv', plk.plk_params(blob, lk_bias, self.kernel_size, products, Sb, M, 0))
            if self.use_ea:
                plan.conv(ops.conv_params(W[f'{p}.ea'], M, h, w, out_f32=G))
                plan.launch('rsa_ea_gate', plk.ea_gate_params(G, M, M, dim))
            if self._norm:
                plan.conv(ops.conv_params(W[f'{p}.refine'], M, h, w, out_f32=R))
                gamma, beta = W[f'{p}.norm']
                ap = plk.group_norm_apply_params(R, dim, NORM_GROUPS, stats, gamma, beta, Xf[xi], X[xo], Xf[xo])
                stats_args = plk.group_norm_stats_args(R, dim, NORM_GROUPS, ws, stats)
                plan.launch((('rsa_group_norm_stats', stats_args), ('rsa_group_norm_apply', ap)), kernels=3)
            else:
                plan.conv(ops.conv_params(W[f'{p}.refine'], M, h, w, res1=Xf[xi], out=X[xo], out_f32=Xf[xo]))

        y = plan.output((n, self.in_ch, h * s, w * s), dtype)
        if getattr(self, 'dysample', False):
            Y = plan.planes(n, (self.in_ch * s * s + 7) // 8, h, w, with_lo)
            plan.conv(ops.conv_params(W['last'], fin, h, w, out=Y))
            dys.emit(plan, W, Y, y)
        else:
            plan.conv(ops.conv_params(W['last'], fin, h, w, out_nchw=y, pixel_shuffle=s, out_base=plan.input_ref(x_shape, dtype)))
        return set_input


class plksr(_PLKBase):  # noqa: N801  (the reference's class name, recorded in the fixtures' metadata)
    """PLKSR (plksr.py:259-323): CCM / ICCM / DCCM mixers with GELU, PLK / SparsePLK / RectSparsePLK, optional EA, no normalisation."""

    _mixer_key = 'channe_mixer'  # sic: the reference's key
    _mixer_act = L.ACT_GELU

    def __init__(self, dim: int = 64, n_blocks: int = 28, upscaling_factor: int = 4, ccm_type: str = 'DCCM', kernel_size: int = 17,
                 split_ratio: float = 0.25, lk_type: str = 'PLK', use_ea: bool = True, in_ch: int = 3) -> None:  # fmt: skip
        super().__init__()
        pdim = int(dim * split_ratio)
        _check_geometry(dim, pdim, kernel_size, in_ch)
        if ccm_type not in _CCM_K:
            raise ValueError(f'Unknown CCM type: {ccm_type}')
        if lk_type not in ('PLK', 'SparsePLK', 'RectSparsePLK'):
            raise ValueError(f'Unknown LK type: {lk_type}')
        if lk_type == 'RectSparsePLK' and (kernel_size // 3) % 2 == 0:
            raise NotImplementedError(f'RectSparsePLK: kernel_size // 3 = {kernel_size // 3} is even (its padding is not "same")')
        if lk_type == 'SparsePLK':
            kernel_size = max([kernel_size] + [(k - 1) * d + 1 for k, d in _SPARSE])
        self.dim, self.pdim, self.n_blocks, self.upscale, self.in_ch = dim, pdim, n_blocks, upscaling_factor, in_ch
        self.ccm_type, self.kernel_size, self.lk_type, self.use_ea = ccm_type, kernel_size, lk_type, use_ea
        k0, k2 = _CCM_K[ccm_type]
        shapes: dict = {'feats.0.weight': (dim, in_ch, 3, 3), 'feats.0.bias': (dim,)}
        for b in range(1, n_blocks + 1):
            p = f'feats.{b}'
            shapes[f'{p}.channe_mixer.0.weight'] = (2 * dim, dim, k0, k0)
            shapes[f'{p}.channe_mixer.0.bias'] = (2 * dim,)
            shapes[f'{p}.channe_mixer.2.weight'] = (dim, 2 * dim, k2, k2)
            shapes[f'{p}.channe_mixer.2.bias'] = (dim,)
            k = kernel_size
            if lk_type == 'PLK':
                shapes[f'{p}.lk.conv.weight'] = (pdim, pdim, k, k)
                shapes[f'{p}.lk.conv.bias'] = (pdim,)
            elif lk_type == 'RectSparsePLK':
                m, nn_ = k, k // 3
                for name, shp in (('mn_conv', (m, nn_)), ('nm_conv', (nn_, m)), ('nn_conv', (nn_, nn_))):
                    shapes[f'{p}.lk.{name}.weight'] = (pdim, pdim, *shp)
                    shapes[f'{p}.lk.{name}.bias'] = (pdim,)
            else:
                for j, (ks, _) in enumerate(_SPARSE):
                    shapes[f'{p}.lk.convs.{j}.weight'] = (pdim, pdim, ks, ks)
                    shapes[f'{p}.lk.convs.{j}.bias'] = (pdim,)
            if use_ea:
                shapes[f'{p}.attn.f.0.weight'] = (dim, dim, 3, 3)
                shapes[f'{p}.attn.f.0.bias'] = (dim,)
            shapes[f'{p}.refine.weight'] = (dim, dim, 1, 1)
            shapes[f'{p}.refine.bias'] = (dim,)
        last = n_blocks + 1
        shapes[f'feats.{last}.weight'] = (in_ch * upscaling_factor**2, dim, 3, 3)
        shapes[f'feats.{last}.bias'] = (in_ch * upscaling_factor**2,)
        build_param_tree(self, shapes)

    def _last_index(self) -> int:
        return self.n_blocks + 1

    def _lk_weights(self, sd, b: int):
        p = f'feats.{b}.lk'
        if self.lk_type == 'PLK':
            return sd[f'{p}.conv.weight'], sd[f'{p}.conv.bias']
        if self.lk_type == 'RectSparsePLK':
            return plk.fold_rect_sparse(*(sd[f'{p}.{c}.{t}'] for c in ('mn_conv', 'nm_conv', 'nn_conv') for t in ('weight', 'bias')), self.kernel_size)
        return plk.fold_sparse([(sd[f'{p}.convs.{j}.weight'], sd[f'{p}.convs.{j}.bias'], d) for j, (_, d) in enumerate(_SPARSE)], self.kernel_size)


class realplksr(_PLKBase):  # noqa: N801
    """RealPLKSR (rplksr.py:108-172): DCCM with Mish, PLK, optional EA, refine, GroupNorm(4) + skip; PixelShuffle or DySample head."""

    # GroupNorm normalises over the WHOLE image: output computed tile by tile differs from the whole-image output (tiling.py warns)
    global_statistics = True
    _norm = True

    def __init__(self, dim: int = 64, n_blocks: int = 28, upscaling_factor: int = 4, kernel_size: int = 17, split_ratio: float = 0.25,
                 use_ea: bool = True, norm_groups: int = NORM_GROUPS, dysample: bool = False, in_ch: int = 3) -> None:  # fmt: skip
        super().__init__()
        pdim = int(dim * split_ratio)
        _check_geometry(dim, pdim, kernel_size, in_ch)
        if norm_groups != NORM_GROUPS:
            raise NotImplementedError(f'RealPLKSR: norm_groups must be {NORM_GROUPS}')
        s = upscaling_factor
        self.dim, self.pdim, self.n_blocks, self.upscale, self.in_ch = dim, pdim, n_blocks, s, in_ch
        self.ccm_type, self.kernel_size, self.lk_type, self.use_ea, self.dysample = 'DCCM', kernel_size, 'PLK', use_ea, dysample
        self.dys_groups = in_ch if s % 2 else 4
        if dysample and (in_ch * s * s) % self.dys_groups:
            raise NotImplementedError('RealPLKSR: DySample channels must divide into groups')
        shapes: dict = {'feats.0.weight': (dim, in_ch, 3, 3), 'feats.0.bias': (dim,)}
        for b in range(1, n_blocks + 1):
            p = f'feats.{b}'
            shapes[f'{p}.channel_mixer.0.weight'] = (2 * dim, dim, 3, 3)
            shapes[f'{p}.channel_mixer.0.bias'] = (2 * dim,)
            shapes[f'{p}.channel_mixer.2.weight'] = (dim, 2 * dim, 3, 3)
            shapes[f'{p}.channel_mixer.2.bias'] = (dim,)
            shapes[f'{p}.lk.conv.weight'] = (pdim, pdim, kernel_size, kernel_size)
            shapes[f'{p}.lk.conv.bias'] = (pdim,)
            if use_ea:
                shapes[f'{p}.attn.f.0.weight'] = (dim, dim, 3, 3)
                shapes[f'{p}.attn.f.0.bias'] = (dim,)
            shapes[f'{p}.refine.weight'] = (dim, dim, 1, 1)
            shapes[f'{p}.refine.bias'] = (dim,)
            shapes[f'{p}.norm.weight'] = (dim,)
            shapes[f'{p}.norm.bias'] = (dim,)
        last = n_blocks + 2  # feats[n_blocks + 1] is Dropout2d: the identity in inference
        cin = in_ch * s * s
        shapes[f'feats.{last}.weight'] = (cin, dim, 3, 3)
        shapes[f'feats.{last}.bias'] = (cin,)
        buffers = {}
        if dysample:
            oc = 2 * self.dys_groups * s * s
            if s != 1:
                shapes['to_img.end_conv.weight'] = (in_ch, cin, 1, 1)
                shapes['to_img.end_conv.bias'] = (in_ch,)
            shapes['to_img.offset.weight'] = (oc, cin, 1, 1)
            shapes['to_img.offset.bias'] = (oc,)
            shapes['to_img.scope.weight'] = (oc, cin, 1, 1)
            buffers['to_img.init_pos'] = dys.dysample_init_pos(s, self.dys_groups)
        build_param_tree(self, shapes, buffers)

    def _last_index(self) -> int:
        return self.n_blocks + 2

    def _lk_weights(self, sd, b: int):
        return sd[f'feats.{b}.lk.conv.weight'], sd[f'feats.{b}.lk.conv.bias']
