"""SMoSR on the MI355X engine (reference module: ``resselt/archs/smosr/arch.py:379-459``), eval-mode semantics.

The network is convolutions and one elementwise tail::

    x = reflect-pad by 2 on all four sides                    rsa_smosr_pad (NCHW -> planes, the pad fused into the read)
    s = short(x)                                              1x1 convolution, written BEHIND the features in the head's input planes
    f = blocks_1(x); f = blocks_2(f) + f; f = end_block(f)    SMB = conv3x3 + SiLU, conv3x3 + SiLU, conv3x3 (C -> 2C) to an f32 map, then
                                                              ONE rsa_smosr_gate launch: (a[:C] + shortcut) * tanh(a[C:]) (+ trunk)
    y = upsampler(cat[s, f]), cropped by 2 * scale            UniUpsampleV4_light

Every convolution but the two kinds of ``short`` is a ``DOConv2d`` (``rep = 0``) or a ``ConvNXC`` (``rep = 1``): over-parameterisations
that ``fold_doconv`` / ``fold_convnxc`` turn into one plain OIHW weight and bias at pack time, in float64, rounded once.  The stored
``eval_conv.*`` tensors are never read (the reference recomputes them from ``W`` / ``D`` / ``mul`` / ``bias`` when it enters eval mode).

``cat[s, f]`` needs no kernel: the input channels of the head's first layer are permuted at pack time so that the features come first;
``end_block.1`` writes planes [0, dim / 8) of the head's input and ``short`` writes from plane dim / 8 on (``out_plane_off``).  A hidden
width of the head that is no multiple of 8 (the nearest+conv head runs at dim + in_ch * scale^2; pixelshuffle at any mid_dim) is padded
with zero weights and biases; DySample's mid_dim channels are laid out so that each of its four groups fills whole units of four
(``dys_layout``), which also makes the width a multiple of 8.

Heads: the five of ``engine/uniupsample.py`` (same layer indices and slopes) on a dict of folded ``{prefix}.{i}.weight / .bias``, DySample
with a 3x3 end convolution sampled in groups of 8 channels, and ``pa_up``: per stage nearest x2 (the convolution's upsample-on-read; at
x3 ``end_block.1`` and ``short`` store every channel 9 times through depth-to-space), conv, rsa_smosr_pa (pixel attention + LeakyReLU
0.2 in one pass on MFMA), conv + LeakyReLU 0.2; then the last convolution.
"""

from __future__ import annotations

import math

import torch

from ...engine import dysample as dys
from ...engine import lib as L
from ...engine import lib_smosr as LS
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ...engine.uniupsample import GROUPS, Head  # (GROUPS: DySample's 4, fixed by SMoSR.__init__ :448)
from ..mosr.arch import _check_dims, _conv_weights

SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'pa_up')
MAX_DIM = 128  # rsa_smosr_gate / rsa_smosr_pa: C up to 128
PAD = 2


# ---- folding (float64 in, float64 out) -------------------------------------------------------------------------------------------------
def fold_doconv(sd, p: str):
    """``DOConv2d`` under the key prefix ``p`` -> (OIHW weight, bias): ``DoW * mul`` and ``bias * mul`` (:261-269), with
    ``DoW[o, i, m] = sum_s (D + d_diag)[i, m, s] W[o, i, s]`` for a k x k kernel and ``W`` itself for 1 x 1."""
    w = sd[f'{p}.W'].double()
    mul = sd[f'{p}.mul'].double().reshape(())
    co, ci, kk = w.shape
    if f'{p}.D' in sd:
        w = torch.einsum('ims,ois->oim', sd[f'{p}.D'].double() + sd[f'{p}.d_diag'].double(), w)
    k = math.isqrt(kk)
    return (w * mul).reshape(co, ci, k, k), sd[f'{p}.bias'].double() * mul


def fold_convnxc(sd, p: str):
    """``ConvNXC`` under ``p`` -> (OIHW weight, bias): the 1x1 -> k x k (valid, on the zero-padded input) -> 1x1 chain composed into one
    k x k kernel, plus the 1x1 ``sk`` at its centre (``update_params`` :320-354)."""
    (w1, b1), (w2, b2), (w3, b3) = (fold_doconv(sd, f'{p}.conv.{i}') for i in range(3))
    ws, bs = fold_doconv(sd, f'{p}.sk')
    w = torch.einsum('oa,abhw,bi->oihw', w3[:, :, 0, 0], w2, w1[:, :, 0, 0])
    b = w3[:, :, 0, 0] @ (torch.einsum('abhw,b->a', w2, b1) + b2) + b3
    k = w.shape[-1]
    w[:, :, k // 2, k // 2] += ws[:, :, 0, 0]
    return w, b + bs


def fold(sd, p: str, rep: bool):
    return fold_convnxc(sd, p) if rep else fold_doconv(sd, p)


# ---- parameter tree --------------------------------------------------------------------------------------------------------------------
def _doconv_shapes(shapes: dict, muls: dict, p: str, ci: int, co: int, k: int, mul: float = 1.0) -> None:
    """DOConv2d's registration order (:225-258): mul, W, (D, d_diag), bias, eval_conv."""
    kk = k * k
    shapes[f'{p}.mul'] = (1,)
    muls[f'{p}.mul'] = mul
    shapes[f'{p}.W'] = (co, ci, kk)
    if kk > 1:
        shapes[f'{p}.D'] = (ci, kk, kk)
        shapes[f'{p}.d_diag'] = (ci, kk, kk)
    shapes[f'{p}.bias'] = (co,)
    shapes[f'{p}.eval_conv.weight'] = (co, ci, k, k)
    shapes[f'{p}.eval_conv.bias'] = (co,)


def _conv_shapes(shapes: dict, muls: dict, p: str, ci: int, co: int, k: int, rep: bool, mul: float = 1.0) -> None:
    """A ``ConvNXC(ci, co, (k, k), mul=mul) if rep else DOConv2d(ci, co, k, mul=mul)`` under ``p`` (ConvNXC :306-317: sk, conv.0-2, eval_conv)."""
    if not rep:
        _doconv_shapes(shapes, muls, p, ci, co, k, mul)
        return
    _doconv_shapes(shapes, muls, f'{p}.sk', ci, co, 1, 0.02)
    _doconv_shapes(shapes, muls, f'{p}.conv.0', ci, 2 * ci, 1)
    _doconv_shapes(shapes, muls, f'{p}.conv.1', 2 * ci, 2 * co, k)
    _doconv_shapes(shapes, muls, f'{p}.conv.2', 2 * co, co, 1, mul)
    shapes[f'{p}.eval_conv.weight'] = (co, ci, k, k)
    shapes[f'{p}.eval_conv.bias'] = (co,)


def pa_layers(scale: int, in_dim: int, out_dim: int, mid_dim: int):
    """The ``pa_up`` head (:140-163): [(index of the stage's first convolution, its cin)], and the last convolution's index."""
    if scale & (scale - 1) and scale != 3:
        raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
    stages = int(math.log2(scale)) if scale & (scale - 1) == 0 else 1
    return [(6 * j + 1, in_dim if j == 0 else mid_dim) for j in range(stages)], 6 * stages


def dys_layout(mid: int):
    """Where DySample's ``mid`` input channels sit in the buffers: rsa_dysample reads each of the four channel groups as whole units of
    four channels, so a group of ``mid / 4`` channels is padded to a multiple of four.  Returns (position of every channel, padded width);
    the identity when ``mid`` is a multiple of 16.  The padded channels carry zero weights and biases everywhere."""
    cpg = mid // GROUPS
    cpg4 = (cpg + 3) // 4 * 4
    c = torch.arange(mid)
    return (c // cpg) * cpg4 + c % cpg, GROUPS * cpg4


def _rows(w: torch.Tensor, pos: torch.Tensor, n: int) -> torch.Tensor:
    """Output channels (dim 0) of a weight or bias moved to ``pos`` in a width of ``n``, zeros elsewhere."""
    out = w.new_zeros((n, *w.shape[1:]))
    out[pos.to(w.device)] = w
    return out


def _cols(w: torch.Tensor, pos: torch.Tensor, n: int) -> torch.Tensor:
    """Input channels (dim 1) likewise."""
    out = w.new_zeros((w.shape[0], n, *w.shape[2:]))
    out[:, pos.to(w.device)] = w
    return out


class SMoSR(EngineModule):
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'fp16')

    def __init__(self, in_ch: int = 3, out_ch: int = 3, dim: int = 48, scale: int = 2, rep: bool = False, n_mb: int = 3,
                 upsampler: str = 'pixelshuffledirect', upsampler_mid_dim: int = 32, d_kernel: int = 3) -> None:  # fmt: skip
        super().__init__()
        if upsampler not in SAMPLE_MODS:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')
        if dim % 8 or dim > MAX_DIM:
            raise NotImplementedError(f'SMoSR: dim must be a multiple of 8 up to {MAX_DIM} (got {dim}; rsa_smosr_gate walks whole planes of a pixel)')
        _check_dims('SMoSR', dim, in_ch)
        if n_mb < 1:
            raise NotImplementedError('SMoSR: at least one block in blocks_2')
        rep, mid, cat = bool(rep), upsampler_mid_dim, dim + in_ch * scale * scale
        if upsampler == 'conv' and scale != 1:
            raise NotImplementedError(f'SMoSR: the conv head with scale {scale} is not built: the reference crops 2 * scale pixels from a map it never '
                                      'upscaled and returns an image smaller than its input')  # fmt: skip
        if upsampler == 'dysample' and scale != 1:
            if rep:
                raise NotImplementedError('SMoSR: rep = 1 with the dysample head is not built: the reference builds ConvNXC(in_dim, out_dim) where '
                                          'mid_dim is meant, and its own forward raises')  # fmt: skip
            if mid == cat:
                raise NotImplementedError('SMoSR: the dysample head with mid_dim == dim + in_ch * scale^2 is not built: the reference\'s loader raises '
                                          'KeyError on upsampler.2.end_conv.weight')  # fmt: skip
            if d_kernel not in (1, 3):
                raise NotImplementedError(f'SMoSR: DySample end kernels of 1 and 3 are built (got {d_kernel})')
        self.pa = upsampler == 'pa_up' and scale != 1
        if self.pa and (mid % 8 or mid > MAX_DIM or mid < 8):
            raise NotImplementedError(f'SMoSR: pa_up needs mid_dim a multiple of 8 up to {MAX_DIM} (got {mid}; rsa_smosr_pa multiplies whole planes)')
        self.in_ch, self.out_ch, self.dim, self.scale, self.rep, self.n_mb = in_ch, out_ch, dim, scale, rep, n_mb
        self.head, self.mid_dim, self.d_kernel, self.cat = upsampler, mid, d_kernel, cat
        shapes: dict = {}
        self._mul_init: dict = {}
        m = self._mul_init
        shapes['short.weight'], shapes['short.bias'] = (cat - dim, in_ch, 1, 1), (cat - dim,)
        self.blocks = ['blocks_1.0', 'blocks_1.1'] + [f'blocks_2.{j}' for j in range(n_mb)] + ['end_block.0']
        for b in self.blocks:
            ci = in_ch if b == 'blocks_1.0' else dim
            if ci != dim:
                shapes[f'{b}.short.weight'], shapes[f'{b}.short.bias'] = (dim, ci, 1, 1), (dim,)
            for i, (a, o) in zip((0, 2, 4), ((ci, dim), (dim, dim), (dim, 2 * dim))):
                _conv_shapes(shapes, m, f'{b}.body.{i}', a, o, 3, rep, mul=3.0)
        _conv_shapes(shapes, m, 'end_block.1', dim, dim, 3, rep)
        # the head: [(key prefix, cin, cout, k)] of its convolutions in module order, the pixel attentions apart
        self.dys_index = self.dys_pos = None
        if self.pa:
            self.pa_stages, self.last_index = pa_layers(scale, cat, out_ch, mid)
            self.head_convs = []
            for i, ci in self.pa_stages:
                self.head_convs += [(i, ci, mid, 3), (i + 1, mid, mid, 1), (i + 3, mid, mid, 3)]
            self.head_convs.append((self.last_index, mid, out_ch, 3))
        else:
            self.up = Head('upsampler', upsampler, scale, cat, out_ch, mid, end_kernel=d_kernel)
            self.dys_index = self.up.dys_index
            self.head_convs = [(i, ci, co, k) for i, co, ci, k in self.up.layers]
        # the width the head's hidden layers RUN at: whole planes (DySample: whole units of four per channel group), zero weights beyond mid
        self.mid_run = mid
        if self.dys_index is not None:
            self.dys_pos, self.mid_run = dys_layout(mid) if mid > GROUPS and mid % GROUPS == 0 else (None, mid)
        elif upsampler == 'pixelshuffle' and scale != 1:
            self.mid_run = (mid + 7) // 8 * 8
        meta_in = mid if self.pa and scale & (scale - 1) == 0 else cat  # (:151: the pa_up loop re-binds in_dim before the buffer is built)
        buffers = {'upsampler.MetaUpsample': torch.tensor([254, SAMPLE_MODS.index(upsampler), scale, meta_in & 0xFF, out_ch, mid & 0xFF, GROUPS, int(rep)], dtype=torch.uint8)}
        for i, ci, co, k in self.head_convs:
            _conv_shapes(shapes, m, self._head_key(i), ci, co, k, rep)
        if self.dys_index is not None:
            if mid <= GROUPS or mid % GROUPS:
                raise ValueError('Incorrect in_channels and groups values.')
            d, s = f'upsampler.{self.dys_index}', scale
            shapes[f'{d}.end_conv.weight'], shapes[f'{d}.end_conv.bias'] = (out_ch, mid, d_kernel, d_kernel), (out_ch,)
            shapes[f'{d}.offset.weight'], shapes[f'{d}.offset.bias'] = (2 * GROUPS * s * s, mid, 1, 1), (2 * GROUPS * s * s,)
            shapes[f'{d}.scope.weight'] = (2 * GROUPS * s * s, mid, 1, 1)
            buffers[f'{d}.init_pos'] = dys.dysample_init_pos(s, GROUPS)
        build_param_tree(self, shapes, buffers)

    def _head_key(self, i: int) -> str:
        """Key prefix of the head's convolution at module index ``i``: a pixel attention (index 6 j + 2) keeps its own in ``conv.0``
        (PA.conv = Sequential(conv, Sigmoid) :81)."""
        return f'upsampler.{i}.conv.0' if self.pa and i % 6 == 2 else f'upsampler.{i}'

    # ---- pack ----
    def folded_state(self, device=None) -> dict:
        """Plain ``{prefix}.weight / .bias`` (float32, folded in float64) of every convolution, plus the tensors that are plain already."""
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        out = {k: v.float() for k, v in sd.items() if '.short.' in k or k.startswith('short.') or f'upsampler.{self.dys_index}.' in k}
        names = [f'{b}.body.{i}' for b in self.blocks for i in (0, 2, 4)] + ['end_block.1']
        for i, _, _, _ in self.head_convs:
            names.append(self._head_key(i))
        for p in names:
            w, b = fold(sd, p, self.rep)
            out[f'{p}.weight'], out[f'{p}.bias'] = w.float(), b.float()
        return out if device is None else {k: v.to(device) for k, v in out.items()}

    def _head_first(self, w: torch.Tensor) -> torch.Tensor:
        """Input channels of the head's first layer from the reference's cat[s, f] order to the buffer's [f, s] order."""
        isq = self.cat - self.dim
        return torch.cat([w[:, isq:], w[:, :isq]], 1)

    def _pack(self, device, products):
        sd = self.folded_state(device)
        cw = lambda w, b, **kw: ops.ConvWeights.from_oihw(w, b, products, device=device, **kw)  # noqa: E731
        s, dim, cat = self.scale, self.dim, self.cat
        x3 = self.pa and s == 3  # end_block.1 and short store every channel 9 times through depth-to-space: the nearest x3 map
        rep9 = lambda t: t.repeat_interleave(9, 0) if x3 else t  # noqa: E731
        W: dict = {'short': cw(rep9(sd['short.weight']), rep9(sd['short.bias'])), 'blocks_1.0.short': cw(sd['blocks_1.0.short.weight'], sd['blocks_1.0.short.bias'])}
        for b in self.blocks:
            for i in (0, 2, 4):
                W[f'{b}.body.{i}'] = cw(sd[f'{b}.body.{i}.weight'], sd[f'{b}.body.{i}.bias'])
        W['end_block.1'] = cw(rep9(sd['end_block.1.weight']), rep9(sd['end_block.1.bias']))
        first = self.head_convs[0][0]
        hw = {}
        for i, ci, co, k in self.head_convs:
            p = self._head_key(i)
            w, b = sd[f'{p}.weight'], sd[f'{p}.bias']
            if i == first:
                w = self._head_first(w)
            hw[i] = (w, b)
        if self.pa:
            for j, (i, _) in enumerate(self.pa_stages):
                W[f'pa{j}.a'] = cw(*hw[i])
                W[f'pa{j}.w'], W[f'pa{j}.b'] = LS.pack_pa_weights(hw[i + 1][0], hw[i + 1][1], int(products), products.fmt, device)
                W[f'pa{j}.c'] = cw(*hw[i + 3])
            W['pa.last'] = cw(*hw[self.last_index])
        else:
            head = {}
            cat8 = (cat + 7) // 8 * 8
            mid, run, last = self.mid_dim, self.mid_run, len(self.head_convs) - 1
            ident = torch.arange(mid)
            for j, (i, ci, co, k) in enumerate(self.head_convs):
                w, b = hw[i]
                if self.head == 'nearest+conv' and s != 1 and j < last and not (s == 3 and j == 0):
                    # the hidden width cat is padded to whole planes with zero weights and biases (LeakyReLU(0) = 0 feeds zero columns)
                    w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, cat8 - co))
                    b = torch.nn.functional.pad(b, (0, cat8 - co))
                elif self.head == 'pixelshuffle' and s != 1 and run != mid:
                    # hidden width mid -> run: PixelShuffle takes output channel c r^2 + k to channel c, so whole channels c >= mid are the
                    # tail rows [mid r^2, run r^2) of a shuffled layer; they are zero and meet zero columns in the next layer
                    if j > 0:
                        w = _cols(w, ident, run)
                    if j < last:
                        r2 = co // mid if j > 0 else 1
                        w, b = _rows(w, torch.arange(mid * r2), run * r2), _rows(b, torch.arange(mid * r2), run * r2)
                elif self.dys_index is not None and s != 1 and run != mid:
                    w, b = _rows(w, self.dys_pos, run), _rows(b, self.dys_pos, run)  # head0: cat -> mid, laid out for rsa_dysample
                head[f'upsampler.{i}.weight'], head[f'upsampler.{i}.bias'] = w, b
            if self.dys_index is not None:
                d = f'upsampler.{self.dys_index}'
                relay = (lambda w: _cols(w, self.dys_pos, run)) if run != mid else (lambda w: w)  # noqa: E731
                for k_ in ('offset.bias', 'init_pos', 'end_conv.bias'):
                    head[f'{d}.{k_}'] = sd[f'{d}.{k_}']
                for k_ in ('offset.weight', 'scope.weight'):
                    head[f'{d}.{k_}'] = relay(sd[f'{d}.{k_}'])
                # (a 3x3 end convolution reads the sampled features in the reference's channel order: the head's selection matrices undo dys_pos)
                head[f'{d}.end_conv.weight'] = sd[f'{d}.end_conv.weight'] if self.up.dys3 else relay(sd[f'{d}.end_conv.weight'])
            self.up.pack(W, head, products, device, run=run, dys_pos=self.dys_pos)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        d, s = self.dim, self.scale
        smb = lambda ci: 9 * ci * d + 9 * d * d + 9 * d * 2 * d  # noqa: E731
        total = self.in_ch * (self.cat - d) + self.in_ch * d + smb(self.in_ch) + (2 + self.n_mb) * smb(d) + 9 * d * d
        if self.pa:
            r = 1
            for j, (_, ci) in enumerate(self.pa_stages):
                r = r * 2 if s != 3 else 3
                total += r * r * (9 * ci * self.mid_dim + self.mid_dim * self.mid_dim + 9 * self.mid_dim * self.mid_dim)
            return total + s * s * 9 * self.mid_dim * self.out_ch
        total += sum(co * ci * k * k for _, ci, co, k in self.head_convs)
        if self.dys_index is not None:
            total += self.mid_dim * 2 * GROUPS * s * s * 2 + s * s * self.d_kernel**2 * self.mid_dim * self.out_ch
        return total

    # ---- plan ----
    def _gate(self, plan: Plan, n, H, Wd, a, s_in, *, s2_in=None, s_out=None, planes=None) -> None:
        """One rsa_smosr_gate launch."""
        gp = LS.SmosrGateParams()
        gp.batch, gp.H, gp.W, gp.C = n, H, Wd, self.dim
        gp.a, gp.s_in = a.data_ptr(), s_in.data_ptr()
        gp.s2_in = None if s2_in is None else s2_in.data_ptr()
        gp.s_out = None if s_out is None else s_out.data_ptr()
        if planes is not None:
            planes.bind(gp, 'out')
            gp.fmt = planes.fmt
        # byte model (csrc/smosr.hip): a (2C), s_in, s2_in read once, the stream and the planes written once
        maps = 3 + (s2_in is not None) + (s_out is not None)
        halves = 0 if planes is None else 2 if planes.lo is not None else 1
        label = f'{"stream" if s_out is not None else "no stream"}, {("no", "hi", "hi + lo")[halves]} planes{", + trunk" if s2_in is not None else ""}, {H}x{Wd}'
        plan.launch('rsa_smosr_gate', gp, meta=dict(kernel='rsa_smosr_gate', flop=0, bytes=n * H * Wd * self.dim * (4 * maps + 2 * halves), label=label))

    def _pa(self, plan: Plan, W, j: int, x: Planes, out: Planes, products) -> None:
        """One rsa_smosr_pa launch: pixel attention + LeakyReLU 0.2 of stage ``j``."""
        pp = LS.SmosrPaParams()
        pp.batch, pp.H, pp.W, pp.C, pp.fmt, pp.products, pp.slope = x.n, x.h, x.w, self.mid_dim, x.fmt, int(products), 0.2
        pp.w_frag, pp.bias = W[f'pa{j}.w'].data_ptr(), W[f'pa{j}.b'].data_ptr()
        x.bind(pp, 'in')
        out.bind(pp, 'out')
        halves = 2 if x.lo is not None else 1
        px, c = x.n * x.h * x.w, self.mid_dim
        plan.launch('rsa_smosr_pa', pp, meta=dict(kernel='rsa_smosr_pa', flop=2 * px * c * c, bytes=px * c * 2 * 2 * halves, label=f'stage {j}, {x.h}x{x.w}'))

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        if h0 <= PAD or w0 <= PAD:
            raise RuntimeError(f'input is too small for the reflect padding of {PAD} ({h0}x{w0}: at least {PAD + 1} pixels in either direction)')
        s, dim, cat = self.scale, self.dim, self.cat
        H, Wd = h0 + 2 * PAD, w0 + 2 * PAD
        pd, catp = dim // 8, (cat + 7) // 8
        with_lo = products == 3
        x_pl = plan.planes(n, 1, H, Wd, with_lo)
        fp = LS.SmosrPadParams()
        fp.batch, fp.C, fp.src_h, fp.src_w, fp.pad, fp.dtype, fp.fmt = n, c, h0, w0, PAD, ops.rsa_dtype(dtype), x_pl.fmt
        x_pl.bind(fp, 'out')
        device = plan.device

        def set_input(x):
            fp.x = x.data_ptr()
            L.launch('rsa_smosr_pad', fp, ops.current_stream_ptr(device))  # the reflect pad on all four sides, fused

        A = plan.f32map(n, 2 * dim, H, Wd)  # body.4: value | gate
        S, T = plan.f32map(n, dim, H, Wd), plan.f32map(n, dim, H, Wd)  # the stream, and the trunk residual (blocks_1's output)
        P, t1, t2 = (plan.planes(n, pd, H, Wd, with_lo) for _ in range(3))
        x3 = self.pa and s == 3
        if x3:
            # the head reads the nearest x3 map: end_block.1 and short store each channel 9 times through depth-to-space
            Hc, Wc = 3 * H, 3 * Wd
            shuf_f = torch.empty((n, dim, Hc, Wc), dtype=torch.float32, device=device)
            shuf_s = torch.empty((n, cat - dim, Hc, Wc), dtype=torch.float32, device=device)
            plan.keep += [shuf_f, shuf_s]
        else:
            Hc, Wc = H, Wd
        cat_pl = plan.planes(n, catp, Hc, Wc, with_lo)

        if x3:
            plan.conv(ops.conv_params(W['short'], x_pl, H, Wd, out_nchw=shuf_s, pixel_shuffle=3))
        else:
            plan.conv(ops.conv_params(W['short'], x_pl, H, Wd, out=cat_pl, out_plane_off=pd))
        plan.conv(ops.conv_params(W['blocks_1.0.short'], x_pl, H, Wd, out_f32=S))
        src = x_pl
        last2 = f'blocks_2.{self.n_mb - 1}'
        for b in self.blocks:
            plan.conv(ops.conv_params(W[f'{b}.body.0'], src, H, Wd, act=L.ACT_SILU, out=t1))
            plan.conv(ops.conv_params(W[f'{b}.body.2'], t1, H, Wd, act=L.ACT_SILU, out=t2))
            plan.conv(ops.conv_params(W[f'{b}.body.4'], t2, H, Wd, out_f32=A))
            if b == 'blocks_1.1':  # its output is the trunk residual: kept in T
                self._gate(plan, n, H, Wd, A, S, s_out=T, planes=P)
            elif b == last2:
                self._gate(plan, n, H, Wd, A, T if self.n_mb == 1 else S, s2_in=T, s_out=S, planes=P)
            elif b == 'end_block.0':  # feeds a convolution alone: no stream
                self._gate(plan, n, H, Wd, A, S, planes=P)
            else:
                self._gate(plan, n, H, Wd, A, T if b == 'blocks_2.0' else S, s_out=S, planes=P)
            src = P
        if x3:
            plan.conv(ops.conv_params(W['end_block.1'], P, H, Wd, out_nchw=shuf_f, pixel_shuffle=3))
            back = Planes(cat_pl.hi[:, pd:], None if cat_pl.lo is None else cat_pl.lo[:, pd:])
            plan.call(lambda: (ops.nchw_to_planes(shuf_f, cat_pl), ops.nchw_to_planes(shuf_s, back)))
            plan.count_launches(2)
        else:
            plan.conv(ops.conv_params(W['end_block.1'], P, H, Wd, out=cat_pl))

        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s), crop_origin=(PAD * s, PAD * s))
        if self.pa:
            t, hh, ww, up = cat_pl, Hc, Wc, not x3
            for j in range(len(self.pa_stages)):
                if up:
                    hh, ww = 2 * hh, 2 * ww
                m1, m2, m3 = (plan.planes(n, self.mid_dim // 8, hh, ww, with_lo) for _ in range(3))
                plan.conv(ops.conv_params(W[f'pa{j}.a'], t, hh, ww, upsample2x=up, out=m1))
                self._pa(plan, W, j, m1, m2, products)
                plan.conv(ops.conv_params(W[f'pa{j}.c'], m2, hh, ww, act=L.ACT_LRELU, act_param=0.2, out=m3))
                t, up = m3, True
            plan.conv(ops.conv_params(W['pa.last'], t, hh, ww, out_nchw=y))
        else:
            self.up.emit(plan, W, cat_pl, None, y, with_lo, run=self.mid_run)
        return set_input
