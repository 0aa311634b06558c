"""MoSR on the MI355X engine (reference module: ``resselt/archs/mosr/arch.py:108-156``), and the parts MoSRv2 shares with it.

A gated block (GatedCNNBlock, arch.py:70-105) is

  norm (rsa_layernorm / rsa_rmsnorm, f32 stream -> planes) -> fc1 3x3 conv -> [ g | i | c ] plane ranges
  -> rsa_gated_dwconv: mish(g) * cat(i, depthwise(c)) in one launch -> fc2 3x3 conv + Mish (+ the residual)

``hidden``, ``conv_channels`` and MoSRv2's branch width are often not multiples of 8, while a kernel works on planes of 8 channels.  At pack
time fc1's output rows are re-laid out (``gate_layout``): the passthrough channels and every depthwise segment start on a plane boundary,
the rows of g get exactly the permutation of cat(i, c), and the gaps are zero rows with zero bias (mish(0) * 0 = 0); fc2 gets the same zero
input columns.

MoSR's residual is ``x + (shortcut - 0.5)`` per block.  The f32 stream carries the accumulated offset instead (LayerNorm is shift-
invariant), and the last block removes it exactly: its fc2 writes an f32 map and rsa_group_norm_apply with statistics (0, 1), gamma 1 and
beta = -0.5 * n_block adds the stream.  The trunk's ``- 0.5`` goes into the bias of its last 1x1 convolution, whose residual is the
shortcut branch (a 1x1 convolution has no zero-padded border, so the fold is exact everywhere).
Heads: ``ps`` (final store through depth-to-space), ``gps`` (the mean over 8 groups of a 3x3 conv is one conv with averaged weights,
folded in f64) and ``dys`` (the shared DySample head).
"""

from __future__ import annotations

import torch

from ...engine import dysample as dys
from ...engine import lib as L
from ...engine import ops, plk
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16

LN_EPS = 1e-6
COMPILED_K = (3, 5, 7, 9, 11)  # odd tap counts rsa_gated_dwconv is built for


# ------------------------------------------------------------------------------------------------------------------ pack-time folds
def gate_layout(groups):
    """Plane layout of cat(i, c) for rsa_gated_dwconv.  ``groups``: [(channels, (kh, kw))] in the reference's channel order, (1, 1) = passthrough.
    Leading passthrough groups are merged; every group then starts on a plane boundary.  Returns (perm, i_planes, segments, planes): perm[j] is
    the padded position of channel j, segments [(planes, kh, kw, first source channel, channels)] are the convolution groups in order."""
    perm, segs = [], []
    i_ch, j = 0, 0
    while j < len(groups) and tuple(groups[j][1]) == (1, 1):
        i_ch += groups[j][0]
        j += 1
    perm += list(range(i_ch))
    pos = 8 * ((i_ch + 7) // 8)
    src = i_ch
    for c, (kh, kw) in groups[j:]:
        if (kh, kw) == (1, 1):
            raise NotImplementedError('a passthrough group after a convolution group')
        planes = (c + 7) // 8
        segs.append((planes, kh, kw, src, c))
        perm += list(range(pos, pos + c))
        pos += 8 * planes
        src += c
    return perm, (i_ch + 7) // 8, segs, pos // 8


def relayout_gate(fc1_w, fc1_b, fc2_w, perm, planes):
    """fc1 (2 hidden rows: g, then cat(i, c)) and fc2 (hidden input columns) in the padded layout (f64): fc1 -> 2 * 8 * planes rows,
    [g permuted | cat(i, c) permuted], fc2 -> 8 * planes input columns."""
    d = torch.float64
    h = len(perm)
    hp = 8 * planes
    idx = torch.tensor(perm, dtype=torch.long, device=fc1_w.device)
    w1 = torch.zeros((2 * hp, *fc1_w.shape[1:]), dtype=d, device=fc1_w.device)
    b1 = torch.zeros((2 * hp,), dtype=d, device=fc1_w.device)
    w1[idx] = fc1_w[:h].to(d)
    w1[hp + idx] = fc1_w[h:].to(d)
    b1[idx] = fc1_b[:h].to(d)
    b1[hp + idx] = fc1_b[h:].to(d)
    w2 = torch.zeros((fc2_w.shape[0], hp, *fc2_w.shape[2:]), dtype=d, device=fc2_w.device)
    w2[:, idx] = fc2_w.to(d)
    return w1, b1, w2


def pad_dw(w, b, planes):
    """Depthwise weights [c, 1, kh, kw] + bias [c] -> f32 [8 planes, kh * kw] and [8 planes], zero past c."""
    c = w.shape[0]
    wt = torch.zeros((8 * planes, w.shape[2] * w.shape[3]), dtype=torch.float32, device=w.device)
    bt = torch.zeros((8 * planes,), dtype=torch.float32, device=w.device)
    wt[:c] = w.reshape(c, -1).to(torch.float32)
    bt[:c] = b.to(torch.float32)
    return wt.contiguous(), bt.contiguous()


def fold_gps(w, b):
    """GPS._geo_ensemble (arch.py:24-28): the mean over the 8 groups of the conv's output channels = one conv with averaged weights (f64)."""
    d = torch.float64
    m = w.shape[0] // 8
    return w.to(d).reshape(8, m, *w.shape[1:]).mean(0), b.to(d).reshape(8, m).mean(0)


def _conv_weights(W):
    """Every ops.ConvWeights of a packed dict, the blocks' included."""
    for v in W.values():
        if isinstance(v, ops.ConvWeights):
            yield v
        elif isinstance(v, dict):
            yield from (w for w in v.values() if isinstance(w, ops.ConvWeights))


def _check_dims(name: str, dim: int, in_ch: int) -> None:
    if dim % 8 or dim < 8:
        raise NotImplementedError(f'{name}: dim must be a multiple of 8 (got {dim})')
    if in_ch < 1 or in_ch > 8:
        raise NotImplementedError(f'{name}: 1 to 8 input channels are built (got {in_ch})')


def _check_k(name: str, k: int) -> None:
    if k not in COMPILED_K:
        raise NotImplementedError(f'{name}: depthwise kernel size {k} is not compiled (odd k in [3, 11])')


# ------------------------------------------------------------------------------------------------------------------ shared plan pieces
class _GatedBase(EngineModule):
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'fp16')
    global_statistics = False
    rms_norm = False
    gate_entry, gate_act = 'rsa_gated_dwconv', None  # the gate's entry point, and the activation of one that takes it (rsa_gfisr_gate)

    def _gate_groups(self):
        raise NotImplementedError

    def _pack_block(self, W, sd, b, products, device):
        """The block ``b`` (key prefix) into ``W[b]``."""
        perm, i_planes, segs, planes = gate_layout(self._gate_groups())
        w1, b1, w2 = relayout_gate(sd[f'{b}.fc1.weight'], sd[f'{b}.fc1.bias'], sd[f'{b}.fc2.weight'], perm, planes)
        f32 = torch.float32
        conv = dict(device=device)
        blk = {}
        if self.rms_norm:
            blk['norm'] = (sd[f'{b}.norm.scale'].reshape(-1).contiguous(), sd[f'{b}.norm.offset'].reshape(-1).contiguous())
            # rsa_rmsnorm writes bf16 planes: in the fp16 mode fc1 reads them in one bf16 product
            blk['fc1'] = ops.ConvWeights.from_oihw(w1.to(f32), b1.to(f32), products if products.fmt == PF_BF16 else 1, fmt=PF_BF16, **conv)
        else:
            blk['norm'] = (sd[f'{b}.norm.weight'].contiguous(), sd[f'{b}.norm.bias'].contiguous())
            blk['fc1'] = ops.ConvWeights.from_oihw(w1.to(f32), b1.to(f32), products, **conv)
        blk['fc2'] = ops.ConvWeights.from_oihw(w2.to(f32), sd[f'{b}.fc2.bias'], products, **conv)
        blk['segs'] = [(pl, kh, kw, *pad_dw(*self._dw_weights(sd, b, s), pl)) for s, (pl, kh, kw, _, _) in enumerate(segs)]
        blk['i_planes'], blk['planes'] = i_planes, planes
        if hasattr(self, '_block_gamma'):
            blk['gamma'] = self._block_gamma(sd, b)
        W[b] = blk

    def _dw_weights(self, sd, b, s):
        raise NotImplementedError

    def _emit_block(self, plan: Plan, blk, n, H, Wd, cur, bufs):
        """norm -> fc1 -> (``_emit_branches``) -> the gate; returns the planes fc2 reads.  ``cur`` None: ``bufs['norm']`` already holds the
        normalised input (MoESR: the kernel that closed the previous block wrote it)."""
        self._emit_norm_fc1(plan, blk, n, H, Wd, cur, bufs)
        self._emit_branches(plan, blk, n, H, Wd, bufs)
        return self._emit_gate(plan, blk, n, H, Wd, bufs)

    def _emit_norm_fc1(self, plan: Plan, blk, n, H, Wd, cur, bufs) -> None:
        N_pl, F_pl = bufs['norm'], bufs['fc1']
        sc, off = blk['norm']
        dim = self.dim
        if cur is None:
            pass
        elif self.rms_norm:
            plan.launch('rsa_rmsnorm', dict(x_f32=cur, batch=n, H=H, W=Wd, C=dim, eps=1e-6, scale=sc, offset=off, out=N_pl))
        else:
            lp = L.LayerNormParams()
            lp.batch, lp.H, lp.W, lp.C, lp.eps = n, H, Wd, dim, LN_EPS
            lp.x_f32, lp.gamma, lp.beta = cur.data_ptr(), sc.data_ptr(), off.data_ptr()
            N_pl.bind(lp, 'out')
            lp.out_fmt = N_pl.fmt
            plan.launch('rsa_layernorm', lp)
        plan.conv(ops.conv_params(blk['fc1'], N_pl, H, Wd, out=F_pl))

    def _emit_branches(self, plan: Plan, blk, n, H, Wd, bufs) -> None:
        """What a family runs in place on fc1's output before the gate reads it (the GFISR family's FourierUnit)."""

    def _emit_gate(self, plan: Plan, blk, n, H, Wd, bufs):
        F_pl, M_pl = bufs['fc1'], bufs['gate']
        hp = blk['planes']
        gp = L.GatedDwConvParams()
        gp.batch, gp.H, gp.W, gp.fmt, gp.i_planes, gp.n_segments = n, H, Wd, F_pl.fmt, blk['i_planes'], len(blk['segs'])
        for s, (pl, kh, kw, wt, bt) in enumerate(blk['segs']):
            gp.seg[s].planes, gp.seg[s].kh, gp.seg[s].kw = pl, kh, kw
            gp.seg[s].weight, gp.seg[s].bias = wt.data_ptr(), bt.data_ptr()
        F_pl.bind(gp, 'g')
        F_pl.bind(gp, 'x', hp)
        M_pl.bind(gp, 'out')
        # byte model: g and cat(i, c) read once, the product written once (the halo re-reads stay on chip)
        unit = 16 * (2 if F_pl.lo is not None else 1)
        args = gp if self.gate_act is None else dict(p=gp, act=self.gate_act)
        plan.launch(self.gate_entry, args, meta=dict(kernel=self.gate_entry, flop=0, bytes=n * H * Wd * unit * 3 * hp))
        return M_pl

    def _block_buffers(self, plan: Plan, n, H, Wd, with_lo):
        perm, i_planes, segs, planes = gate_layout(self._gate_groups())
        pd = self.dim // 8
        if self.rms_norm:  # (rsa_rmsnorm writes bf16 planes; no lo halves in the fp16 mode, whose fc1 takes one bf16 product)
            norm = plan.planes(n, pd, H, Wd, with_lo, fmt=PF_BF16)
        else:
            norm = plan.planes(n, pd, H, Wd, with_lo)
        return dict(norm=norm, fc1=plan.planes(n, 2 * planes, H, Wd, with_lo), gate=plan.planes(n, planes, H, Wd, with_lo))

    @staticmethod
    def _unit_stats(n, dev):
        st = torch.zeros((n, 1, 2), dtype=torch.float32, device=dev)
        st[..., 1] = 1.0
        return st

    def _trunk_tail(self, W, sd, first, products, device):
        t = first + self.n_block
        for k, name in ((t, 'tail0'), (t + 2, 'tail1')):
            W[name] = ops.ConvWeights.from_oihw(sd[f'gblocks.{k}.weight'], sd[f'gblocks.{k}.bias'], products, device=device)
        return t + 4


class mosr(_GatedBase):  # noqa: N801  (the reference's class name, recorded in the fixtures' metadata)
    """MoSR (mosr/arch.py:108-156): LayerNorm blocks with a k x k depthwise conv of conv_channels, ConvBlock shortcut, ps / dys / gps head."""

    def __init__(self, in_ch: int = 3, out_ch: int = 3, upscale: int = 4, n_block: int = 24, dim: int = 64, upsampler: str = 'ps', kernel_size: int = 7,
                 expansion_ratio: float = 1.5, conv_ratio: float = 1.0) -> None:  # fmt: skip
        super().__init__()
        if upsampler == 'ps':
            out_ch = in_ch
        if upsampler not in ('ps', 'dys', 'gps'):
            raise NotImplementedError(f'upsampler: {upsampler} not supported')
        _check_dims('MoSR', dim, in_ch)
        _check_k('MoSR', kernel_size)
        if n_block < 1:
            raise NotImplementedError('MoSR: at least one block')
        hidden = int(expansion_ratio * dim)
        cc = int(conv_ratio * dim)
        if cc < 1 or cc > hidden:
            raise NotImplementedError(f'MoSR: conv channels must be in [1, hidden] (got {cc})')
        self.in_ch, self.out_ch, self.upscale, self.n_block, self.dim = in_ch, out_ch, upscale, n_block, dim
        self.head, self.kernel_size, self.hidden, self.conv_channels = upsampler, kernel_size, hidden, cc
        if upsampler == 'dys' and (dim <= 4 or dim % 4):
            raise ValueError('Incorrect in_channels and groups values.')
        shapes: dict = {'gblocks.0.weight': (dim, in_ch, 3, 3), 'gblocks.0.bias': (dim,)}
        for i in range(1, n_block + 1):
            b = f'gblocks.{i}'
            shapes[f'{b}.norm.weight'] = (dim,)
            shapes[f'{b}.norm.bias'] = (dim,)
            shapes[f'{b}.fc1.weight'] = (2 * hidden, dim, 3, 3)
            shapes[f'{b}.fc1.bias'] = (2 * hidden,)
            shapes[f'{b}.conv.weight'] = (cc, 1, kernel_size, kernel_size)
            shapes[f'{b}.conv.bias'] = (cc,)
            shapes[f'{b}.fc2.weight'] = (dim, hidden, 3, 3)
            shapes[f'{b}.fc2.bias'] = (dim,)
        t = n_block + 1
        for k, (co, ci, ks) in ((t, (2 * dim, dim, 3)), (t + 2, (dim, 2 * dim, 3)), (t + 4, (dim, dim, 1))):
            shapes[f'gblocks.{k}.weight'] = (co, ci, ks, ks)
            shapes[f'gblocks.{k}.bias'] = (co,)
        for name, (co, ci, ks) in (('block.0', (dim, in_ch, 3)), ('block.2', (dim, dim, 3)), ('conv11', (dim, in_ch, 1))):
            shapes[f'shortcut.{name}.weight'] = (co, ci, ks, ks)
            shapes[f'shortcut.{name}.bias'] = (co,)
        buffers = {}
        s = upscale
        if upsampler == 'ps':
            shapes['upsampler.0.weight'] = (out_ch * s * s, dim, 3, 3)
            shapes['upsampler.0.bias'] = (out_ch * s * s,)
        elif upsampler == 'gps':
            shapes['upsampler.in_to_k.weight'] = (s * s * out_ch * 8, dim, 3, 3)
            shapes['upsampler.in_to_k.bias'] = (s * s * out_ch * 8,)
        else:
            oc = 8 * s * s
            shapes['upsampler.end_conv.weight'] = (out_ch, dim, 1, 1)
            shapes['upsampler.end_conv.bias'] = (out_ch,)
            shapes['upsampler.offset.weight'] = (oc, dim, 1, 1)
            shapes['upsampler.offset.bias'] = (oc,)
            shapes['upsampler.scope.weight'] = (oc, dim, 1, 1)
            buffers['upsampler.init_pos'] = dys.dysample_init_pos(s, 4)
        build_param_tree(self, shapes, buffers)

    def _gate_groups(self):
        h, cc, k = self.hidden, self.conv_channels, self.kernel_size
        return [(h - cc, (1, 1)), (cc, (k, k))] if h > cc else [(cc, (k, k))]

    def _dw_weights(self, sd, b, s):
        return sd[f'{b}.conv.weight'], sd[f'{b}.conv.bias']

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        dim, s = self.dim, self.upscale
        cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
        W: dict = {'conv0': cw(sd['gblocks.0.weight'], sd['gblocks.0.bias'])}
        for i in range(1, self.n_block + 1):
            self._pack_block(W, sd, f'gblocks.{i}', products, device)
        last = self._trunk_tail(W, sd, 1, products, device)
        W['tail2'] = cw(sd[f'gblocks.{last}.weight'], sd[f'gblocks.{last}.bias'] - 0.5)  # + (shortcut(x) - 0.5): the offset in the 1x1's bias
        W['sc0'] = cw(sd['shortcut.block.0.weight'], sd['shortcut.block.0.bias'])
        W['sc2'] = cw(sd['shortcut.block.2.weight'], sd['shortcut.block.2.bias'])
        W['sc11'] = cw(sd['shortcut.conv11.weight'], sd['shortcut.conv11.bias'])
        W['gamma1'] = torch.ones(dim, dtype=torch.float32, device=device)
        W['beta_off'] = torch.full((dim,), -0.5 * self.n_block, dtype=torch.float32, device=device)
        if self.head == 'ps':
            W['up'] = cw(sd['upsampler.0.weight'], sd['upsampler.0.bias'])
        elif self.head == 'gps':
            w, b = fold_gps(sd['upsampler.in_to_k.weight'], sd['upsampler.in_to_k.bias'])
            W['up'] = cw(w.to(torch.float32), b.to(torch.float32))
        else:
            dys.pack(W, sd['upsampler.offset.weight'], sd['upsampler.offset.bias'], sd['upsampler.scope.weight'],
                     sd['upsampler.end_conv.weight'].reshape(self.out_ch, dim), sd['upsampler.end_conv.bias'], sd['upsampler.init_pos'], 4, s,
                     products=products, device=device)  # fmt: skip
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        d, h, s, k = self.dim, self.hidden, self.upscale, self.kernel_size
        blk = 9 * d * 2 * h + k * k * self.conv_channels + 9 * h * d
        head = 9 * d * self.out_ch * s * s if self.head != 'dys' else d * 8 * s * s * 2
        return 9 * self.in_ch * d + self.n_block * blk + 9 * d * 2 * d * 2 + d * d + 9 * self.in_ch * d + 9 * d * d + self.in_ch * d + head

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, h, w = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        dim, s = self.dim, self.upscale
        pd = dim // 8
        with_lo = products == 3
        dev = plan.device
        x_pl = plan.planes(n, 1, h, w, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)

        cur, nxt = plan.f32map(n, dim, h, w), plan.f32map(n, dim, h, w)
        R = plan.f32map(n, dim, h, w)
        feat = plan.planes(n, pd, h, w, with_lo)
        bufs = self._block_buffers(plan, n, h, w, with_lo)
        stats = self._unit_stats(n, dev)
        plan.keep.append(stats)
        plan.conv(ops.conv_params(W['conv0'], x_pl, h, w, out_f32=cur))
        for i in range(1, self.n_block + 1):
            blk = W[f'gblocks.{i}']
            m = self._emit_block(plan, blk, n, h, w, cur, bufs)
            if i < self.n_block:  # the stream carries +0.5 per block (see the module docstring)
                plan.conv(ops.conv_params(blk['fc2'], m, h, w, act=L.ACT_MISH, res1=cur, alpha=1.0, out_f32=nxt))
                cur, nxt = nxt, cur
            else:
                plan.conv(ops.conv_params(blk['fc2'], m, h, w, act=L.ACT_MISH, out_f32=R))
                ap = plk.group_norm_apply_params(R, dim, 1, stats, W['gamma1'], W['beta_off'], cur, feat, None)
                plan.launch('rsa_group_norm_apply', ap)
        # trunk tail and the ConvBlock shortcut
        t1 = plan.planes(n, 2 * pd, h, w, with_lo)
        t2 = plan.planes(n, pd, h, w, with_lo)
        s1 = plan.planes(n, pd, h, w, with_lo)
        e11 = plan.f32map(n, dim, h, w)
        plan.conv(ops.conv_params(W['tail0'], feat, h, w, act=L.ACT_MISH, out=t1))
        plan.conv(ops.conv_params(W['tail1'], t1, h, w, act=L.ACT_MISH, out=t2))
        plan.conv(ops.conv_params(W['sc0'], x_pl, h, w, act=L.ACT_MISH, out=s1))
        plan.conv(ops.conv_params(W['sc11'], x_pl, h, w, out_f32=e11))
        plan.conv(ops.conv_params(W['sc2'], s1, h, w, act=L.ACT_MISH, res1=e11, alpha=1.0, out_f32=R))
        fe = plan.planes(n, pd, h, w, with_lo)
        fe32 = None
        if self.head == 'dys' and dys.needs_f32_input(W):
            fe32 = plan.f32map(n, dim, h, w)
        plan.conv(ops.conv_params(W['tail2'], t2, h, w, res1=R, alpha=1.0, out=fe, out_f32=fe32))
        y = plan.output((n, self.out_ch, h * s, w * s), dtype)
        if self.head == 'dys':
            dys.emit(plan, W, fe, y, fe32)
        else:
            plan.conv(ops.conv_params(W['up'], fe, h, w, out_nchw=y, pixel_shuffle=s))
        return set_input
