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

The FourierUnit's packing and its four launches are ``engine/fourier.py``'s (FIGSR's too).  The DFT tables depend on (H, W) alone;
``_build_plan`` builds them once per plan (a plan is cached per input size) in float64.
Trunk: in_to_dim 3x3, the blocks, conv dim -> 2 dim + SiLU, conv 2 dim -> dim, + in_to_dim's output.  No padding anywhere: H and W are
arbitrary.  Head: UniUpsampleV3's conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample (3x3 end convolution) through
``engine/uniupsample.py``; transpose+conv, lda and pa_up are refused.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import ops, plk
from ...engine.base import Plan, check_fp16_range
from ...engine.fourier import EPS, dft_workspace, emit_fourier_unit, pack_fourier_unit
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16
from ...engine.uniupsample import SAMPLE_MODS, SAMPLE_MODS3, Head, OwnMetaUpsample
from ..mosr.arch import _check_dims, _conv_weights, _GatedBase, pad_dw, relayout_gate

MAX_DIM = 128  # rsa_gfisr_dft: at most 128 channels per transform
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


class GFISRV2(OwnMetaUpsample, _GatedBase):  # (the reference's load_state_dict override: arch.py:678-680)
    rms_norm = True
    global_statistics = True  # the FourierUnit spans the whole tensor it is given: a tile computes what the reference computes on that tile
    gate_entry, gate_act = 'rsa_gfisr_gate', L.ACT_SILU

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
        self.up = Head('upscale', upsampler, scale, dim, out_nc, mid_dim, end_kernel=3, version=3)
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
        buffers: dict = {}
        self.up.shapes(shapes, buffers, whole_planes='GFISRv2')
        build_param_tree(self, shapes, buffers)

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
        # to the gate the FourierUnit's planes [f0, f0 + f_pl) are part of the passthrough range
        blk['i_planes'], blk['f0'], blk['planes'] = i_pl + f_pl, i_pl, planes
        blk['gamma'] = sd[f'{b}.gamma'].reshape(-1).contiguous()
        fu = f'{b}.conv.{next(name for name, kind in branch_order(shift) if kind is None)}'
        norm = lambda name: (sd[f'{fu}.{name}.scale'].reshape(-1), sd[f'{fu}.{name}.offset'].reshape(-1), EPS)  # noqa: E731
        blk.update(pack_fourier_unit(sd, fu, cf, norm('rn'), norm('post_norm'), device))
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
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    def macs_per_input_pixel(self) -> int:
        """Convolution and depthwise MACs per pixel; the dense DFT is not a per-pixel cost (O(H + W) per pixel) and is left out."""
        d, h, cf = self.dim, self.hidden, self.cf
        blk = 9 * d * 2 * h + (9 + 22) * self.gc + 9 * h * d + 2 * cf * 2 * cf + 9 * 2 * cf
        return 9 * self.in_ch * d + self.n_block * blk + 9 * d * 2 * d * 2 + self.up.macs()

    # ---------------------------------------------------------------- plan
    def _emit_branches(self, plan: Plan, blk, n, H, Wd, bufs) -> None:
        emit_fourier_unit(plan, blk, bufs['dft'], n, H, Wd, self.cf, bufs['fc1'], blk['planes'] + blk['f0'], bufs['spec'], bufs['sp'])

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
        bufs = dict(norm=plan.planes(n, pd, H, Wd, with_lo, fmt=PF_BF16), fc1=plan.planes(n, 2 * hp, H, Wd, with_lo), gate=plan.planes(n, hp, H, Wd, with_lo),
                    spec=plan.f32map(n, 2 * cf, H, Wf), sp=plan.planes(n, (2 * cf + 7) // 8, H, Wf, True, fmt=PF_BF16),
                    dft=dft_workspace(plan, 'GFISRv2', n, cf, H, Wd))  # fmt: skip
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
        fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None
        plan.conv(ops.conv_params(W['tail0'], feat, H, Wd, act=L.ACT_SILU, out=t1))
        plan.conv(ops.conv_params(W['tail1'], t1, H, Wd, res1=trunk, alpha=1.0, out=fe, out_f32=fe32))
        # (the reference crops to 4 H x 4 W whatever the scale: nothing for scales up to 4)
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype)
        self.up.emit(plan, W, fe, fe32, y, with_lo)
        return set_input
