"""GateR on the MI355X engine (reference module: ``resselt/archs/gater/arch.py:162-200``), eval-mode semantics.

A U-shaped x1 restoration network of gated blocks at four resolutions (``dim`` channels at full resolution, ``8 dim`` at 1/8).  A block is

  rsa_rmsnorm_torch (f32 stream -> planes) -> fc1 (a Linear = 1x1 convolution) -> [ g | i | c ] plane ranges
  -> rsa_gated_dwconv: mish(g) * cat(i, dw7x7(c)) in one launch -> fc2 (1x1) + the stream in its epilogue, f32 map out

as in MoSR (``archs/mosr/arch.py``), whose pack-time plane layout of fc1 / fc2 it reuses.  The residual stream between blocks stays an f32 map.
With ``latent_att`` the 1/8-resolution blocks replace the depthwise convolution by FLPVT2, a focused linear attention over ALL tokens:

  q | k | v = one 3C-wide 1x1 convolution of c (the q and kv weights merged at pack time)
  -> rsa_fla_reduce (per-head k^T v / n and mean(k): partial sums per token chunk, added in a fixed order, no atomics)
  -> rsa_fla_apply (focus q, (q KV) z, + the 5x5 depthwise convolution of v)  -> proj (1x1), written over c's planes of the fc1 buffer
  -> rsa_gated_dwconv with no convolution segment: mish(g) * cat(i, proj)

Downsample = 3x3 convolution (f32 map out) + rsa_pixel_unshuffle2 into the next level's stream; Upsample = 3x3 convolution stored through
depth-to-space + the layout kernel that writes its planes INTO the decoder's concatenation buffer, whose other half the encoder's last block
wrote -- the 1x1 convolutions of dec0 / dec1 read the concatenation without a copy.  dec2 has no such convolution: its stream is
cat(dec1, enc0) as an f32 map, built by rsa_f32map_concat from the depth-to-space store and enc0's stream in the launch dec1's layout change
needs anyway.  The input's reflect pad is fused into rsa_nchw_to_planes; ``+ x`` on the padded input is rsa_bilinear_add at scale 1 (exact)
over the cropped region.  The caller's input is never written.
"""

from __future__ import annotations

from fractions import Fraction

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ..mosr.arch import _conv_weights, gate_layout, pad_dw, relayout_gate

BLOCK_LIST = ('enc0', 'enc1.1', 'enc2.1', 'latent.1', 'dec0.1', 'dec1.1', 'dec2.0')
LEVELS = (0, 1, 2, 3, 2, 1, 0)  # resolution level (1 / 2^level) of each entry of BLOCK_LIST
HEADS = 8
BUILT_DIMS = (24, 48)
RMS_EPS = 1e-6


def _view(p: Planes, plane0: int, planes: int) -> Planes:
    """Planes [plane0, plane0 + planes) of a buffer as a buffer of its own (same storage and strides)."""
    lo = p.lo[:, plane0 : plane0 + planes] if p.has_lo(plane0, planes) else None
    return Planes(p.hi[:, plane0 : plane0 + planes], lo)


class GateR(EngineModule):
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')

    def __init__(self, dim: int = 48, in_ch: int = 3, num_blocks=(3, 6, 6, 10, 6, 6, 3), latent_att: bool = False) -> None:
        super().__init__()
        dim, in_ch = int(dim), int(in_ch)
        if dim % 24 or dim < 24:
            raise NotImplementedError(f'GateR: dim must be a multiple of 24 (hidden = int(8/3 * width) must fill planes of 8 channels at all four widths); got {dim}')
        if dim not in BUILT_DIMS:
            raise NotImplementedError(f'GateR: dim {dim} is not built: the latent attention kernels are compiled for head dimensions {BUILT_DIMS} (dim = head dimension)')
        if in_ch < 1 or in_ch > 8:
            raise NotImplementedError(f'GateR: 1 to 8 input channels are built (got {in_ch})')
        num_blocks = tuple(int(b) for b in num_blocks)
        if len(num_blocks) != 7 or min(num_blocks) < 1:
            raise NotImplementedError(f'GateR: seven stages of at least one block each (got {num_blocks})')
        self.dim, self.in_ch, self.num_blocks, self.latent_att = dim, in_ch, num_blocks, bool(latent_att)
        s = ParamShapes()
        s.conv('in_to_dim', dim, in_ch, 3)
        widths = self.widths()
        for j, (name, nb) in enumerate(zip(BLOCK_LIST, num_blocks)):
            w = widths[j]
            if name in ('enc1.1', 'enc2.1', 'latent.1'):  # Downsample: n_feat -> n_feat / 2, then PixelUnshuffle(2)
                s.conv(f'{name[:-2]}.0.body.0', w // 4, w // 2, 3)
            if name in ('dec0.1', 'dec1.1'):
                s.conv(f'{name[:-2]}.0', w, 2 * w, 1)
            att = self.latent_att and name == 'latent.1'
            hidden = self.hidden(w, att)
            for i in range(nb):
                b = f'{name}.gated.{i}'
                s[f'{b}.norm.weight'] = (w,)
                s.linear(f'{b}.fc1', 2 * hidden, w)
                if att:
                    s[f'{b}.conv.focusing_factor'] = (w,)
                    s[f'{b}.conv.scale'] = (w,)
                    s.linear(f'{b}.conv.q', w, w)
                    s.linear(f'{b}.conv.kv', 2 * w, w)
                    s.linear(f'{b}.conv.proj', w, w)
                    s[f'{b}.conv.dwc.weight'] = (w // HEADS, 1, 5, 5)
                    s[f'{b}.conv.dwc.bias'] = (w // HEADS,)
                else:
                    s[f'{b}.conv.conv.weight'] = (w, 1, 7, 7)
                    s[f'{b}.conv.conv.bias'] = (w,)
                s.linear(f'{b}.fc2', w, hidden)
            if name in ('latent.1', 'dec0.1', 'dec1.1'):  # Upsample: n_feat -> 2 n_feat, then PixelShuffle(2)
                s.conv(f'{name[:-2]}.2.body.0', 2 * w, w, 3)
        s.conv('dim_to_ch.0', dim, 2 * dim, 3)
        s.conv('dim_to_ch.1', in_ch, dim, 3)
        build_param_tree(self, s)

    def widths(self):
        d = self.dim
        return (d, 2 * d, 4 * d, 8 * d, 4 * d, 2 * d, 2 * d)  # (dec2 runs on the concatenation: 2 dim at full resolution)

    @staticmethod
    def hidden(width: int, att: bool) -> int:
        return int((1.5 if att else 8 / 3) * width)

    # ---- accounting ----
    def macs_per_input_pixel(self) -> int:
        """Multiply-accumulates per pixel of the padded input: linear layers, convolutions, depthwise taps and the attention's two d x d
        products per head (k^T v and q KV), each at its own resolution."""
        d = self.dim
        total = Fraction(9 * self.in_ch * d + 9 * 2 * d * d + 9 * d * self.in_ch)
        widths = self.widths()
        for j, (name, nb) in enumerate(zip(BLOCK_LIST, self.num_blocks)):
            w, px = widths[j], Fraction(1, 4 ** LEVELS[j])
            att = self.latent_att and name == 'latent.1'
            h = self.hidden(w, att)
            blk = w * 2 * h + h * w
            blk += (3 * w * w + w * w + 25 * w + 2 * w * (w // HEADS)) if att else 49 * w
            total += nb * blk * px
            if name in ('enc1.1', 'enc2.1', 'latent.1'):
                total += 9 * (w // 2) * (w // 4) * px * 4  # the Downsample convolution runs one level up
            if name in ('dec0.1', 'dec1.1'):
                total += 2 * w * w * px
            if name in ('latent.1', 'dec0.1', 'dec1.1'):
                total += 9 * w * 2 * w * px
        return int(total)

    # ---- pack ----
    def _pack_block(self, W, sd, b, width, att, products, device):
        f32 = torch.float32
        hidden = self.hidden(width, att)
        groups = [(hidden, (1, 1))] if att else [(hidden - width, (1, 1)), (width, (7, 7))]
        perm, i_planes, segs, planes = gate_layout(groups)
        lin = lambda k: sd[f'{b}.{k}'].reshape(*sd[f'{b}.{k}'].shape, 1, 1)  # noqa: E731
        w1, b1, w2 = relayout_gate(lin('fc1.weight'), sd[f'{b}.fc1.bias'], lin('fc2.weight'), perm, planes)
        cw = lambda w, bias: ops.ConvWeights.from_oihw(w.to(f32), bias.to(f32), products, device=device)  # noqa: E731
        blk = dict(norm=sd[f'{b}.norm.weight'].contiguous(), fc1=cw(w1, b1), fc2=cw(w2, sd[f'{b}.fc2.bias']), i_planes=i_planes, planes=planes, att=att)
        if att:
            blk['qkv'] = cw(torch.cat((lin('conv.q.weight'), lin('conv.kv.weight')), 0), torch.cat((sd[f'{b}.conv.q.bias'], sd[f'{b}.conv.kv.bias']), 0))
            blk['proj'] = cw(lin('conv.proj.weight'), sd[f'{b}.conv.proj.bias'])
            blk['scale'] = sd[f'{b}.conv.scale'].contiguous()
            blk['factor'] = sd[f'{b}.conv.focusing_factor'].contiguous()
            blk['dwc_w'] = sd[f'{b}.conv.dwc.weight'].reshape(width // HEADS, 25).contiguous()
            blk['dwc_b'] = sd[f'{b}.conv.dwc.bias'].contiguous()
            blk['segs'] = []
        else:
            blk['segs'] = [(pl, kh, kw, *pad_dw(sd[f'{b}.conv.conv.weight'], sd[f'{b}.conv.conv.bias'], pl)) for pl, kh, kw, _, _ in segs]
        W[b] = blk

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        cw = lambda name: ops.ConvWeights.from_oihw(sd[f'{name}.weight'], sd[f'{name}.bias'], products, device=device)  # noqa: E731
        W: dict = {name: cw(name) for name in ('in_to_dim', 'enc1.0.body.0', 'enc2.0.body.0', 'latent.0.body.0', 'latent.2.body.0', 'dec0.0', 'dec0.2.body.0',
                                              'dec1.0', 'dec1.2.body.0', 'dim_to_ch.0', 'dim_to_ch.1')}  # fmt: skip
        widths = self.widths()
        for j, (name, nb) in enumerate(zip(BLOCK_LIST, self.num_blocks)):
            for i in range(nb):
                self._pack_block(W, sd, f'{name}.gated.{i}', widths[j], self.latent_att and name == 'latent.1', products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    # ---- plan ----
    def _emit_block(self, plan: Plan, blk, n, H, Wd, width, cur, bufs):
        """norm -> fc1 -> (attention ->) gate; returns the planes fc2 reads."""
        N_pl, F_pl, M_pl = bufs['norm'], bufs['fc1'], bufs['gate']
        geo = dict(batch=n, H=H, W=Wd, fmt=N_pl.fmt)
        unit = 16 * (2 if N_pl.lo is not None else 1)
        plan.launch('rsa_rmsnorm_torch', dict(x_f32=cur, C=width, eps=RMS_EPS, weight=blk['norm'], out=N_pl, **geo),
                    meta=dict(kernel='rsa_rmsnorm_torch', flop=0, bytes=n * H * Wd * (4 * width + unit * (width // 8))))  # fmt: skip
        plan.conv(ops.conv_params(blk['fc1'], N_pl, H, Wd, out=F_pl))
        hp = blk['planes']
        if blk['att']:
            cp = width // 8
            c0 = 2 * hp - cp  # c's planes in the fc1 buffer: [g | i | c]
            Q_pl, A_pl, ws = bufs['qkv'], bufs['attn'], bufs['ws']
            plan.conv(ops.conv_params(blk['qkv'], F_pl, H, Wd, in_plane0=c0, out=Q_pl))
            d = width // HEADS
            common = dict(qkv=Q_pl, head_dim=d, scale=blk['scale'], factor=blk['factor'], workspace=ws, workspace_bytes=ws.numel() * 4, **geo)
            rec = 4 * (HEADS * d * d + HEADS * d)
            tokens = H * Wd

            # byte model: k and v read once, one partial record per chunk written and read, the finished record written; then q and v read
            # once (the halo re-reads of v stay on chip), the record read once per image, the output planes written
            chunks = (tokens + 127) // 128
            plan.launch('rsa_fla_reduce', common, kernels=2,
                        meta=dict(kernel='rsa_fla_reduce', flop=2 * n * tokens * width * d, bytes=n * (tokens * 2 * cp * unit + (2 * chunks + 1) * rec)))  # fmt: skip
            plan.launch('rsa_fla_apply', dict(dwc_weight=blk['dwc_w'], dwc_bias=blk['dwc_b'], out=A_pl, **common),
                        meta=dict(kernel='rsa_fla_apply', flop=2 * n * tokens * (width * d + 25 * width), bytes=n * (tokens * 3 * cp * unit + rec)))  # fmt: skip
            plan.conv(ops.conv_params(blk['proj'], A_pl, H, Wd, out=F_pl, out_plane_off=c0))
        gp = L.GatedDwConvParams()
        gp.batch, gp.H, gp.W, gp.fmt, gp.i_planes, gp.n_segments = n, H, Wd, F_pl.fmt, blk['i_planes'], len(blk['segs'])
        for s, (pl, kh, kw, wt, bt) in enumerate(blk['segs']):
            gp.seg[s].planes, gp.seg[s].kh, gp.seg[s].kw = pl, kh, kw
            gp.seg[s].weight, gp.seg[s].bias = wt.data_ptr(), bt.data_ptr()
        F_pl.bind(gp, 'g')
        F_pl.bind(gp, 'x', hp)
        M_pl.bind(gp, 'out')
        plan.launch('rsa_gated_dwconv', gp, meta=dict(kernel='rsa_gated_dwconv', flop=0, bytes=n * H * Wd * unit * 3 * hp))
        return M_pl

    def _block_bufs(self, plan: Plan, n, H, Wd, width, att, with_lo, cache):
        key = (width, H, Wd, att)
        if key not in cache:
            hp = self.hidden(width, att) // 8
            b = dict(norm=plan.planes(n, width // 8, H, Wd, with_lo), fc1=plan.planes(n, 2 * hp, H, Wd, with_lo), gate=plan.planes(n, hp, H, Wd, with_lo))
            if att:
                b['qkv'] = plan.planes(n, 3 * width // 8, H, Wd, with_lo)
                b['attn'] = plan.planes(n, width // 8, H, Wd, with_lo)
                nbytes = int(L.load().rsa_fla_workspace_bytes(n, H * Wd, width // HEADS))
                if nbytes <= 0:
                    raise RuntimeError('rsa_fla_workspace_bytes refused the latent grid')
                b['ws'] = torch.empty(nbytes // 4, dtype=torch.float32, device=plan.device)
                plan.keep.append(b['ws'])
            cache[key] = b
        return cache[key]

    def _stage(self, plan: Plan, W, j, n, H, Wd, cur, with_lo, cache, out: Planes, out_plane_off: int = 0, out_f32: bool = False):
        """The blocks of BLOCK_LIST[j] on the f32 stream ``cur``; the last block also writes ``out`` planes.  Returns the final stream map (only
        valid with ``out_f32``)."""
        name, nb, width = BLOCK_LIST[j], self.num_blocks[j], self.widths()[j]
        att = self.latent_att and name == 'latent.1'
        bufs = self._block_bufs(plan, n, H, Wd, width, att, with_lo, cache)
        nxt = plan.f32map(n, width, H, Wd)
        for i in range(nb):
            blk = W[f'{name}.gated.{i}']
            m = self._emit_block(plan, blk, n, H, Wd, width, cur, bufs)
            if i < nb - 1:
                plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, res1=cur, alpha=1.0, out_f32=nxt))
            else:
                plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, res1=cur, alpha=1.0, out=out, out_plane_off=out_plane_off, out_f32=nxt if out_f32 else None))
            cur, nxt = nxt, cur
        return cur

    def _down(self, plan: Plan, wts, src: Planes, in_plane0, n, H, Wd, width_out):
        """Downsample: 3x3 convolution (f32 map) + PixelUnshuffle(2) into a new stream of ``width_out`` channels at H/2 x W/2."""
        t = plan.f32map(n, width_out // 4, H, Wd)
        s = plan.f32map(n, width_out, H // 2, Wd // 2)
        plan.conv(ops.conv_params(wts, src, H, Wd, in_plane0=in_plane0, out_f32=t))
        plan.launch('rsa_pixel_unshuffle2', dict(x_f32=t, batch=n, H=H, W=Wd, C=width_out // 4, out_f32=s),
                    meta=dict(kernel='rsa_pixel_unshuffle2', flop=0, bytes=2 * n * H * Wd * width_out))  # fmt: skip
        return s

    def _up(self, plan: Plan, wts, src: Planes, n, H, Wd, width_in):
        """Upsample: 3x3 convolution to 2 width_in channels stored through depth-to-space: f32 [n, width_in / 2, 2H, 2W]."""
        shuffled = torch.empty((n, width_in // 2, 2 * H, 2 * Wd), dtype=torch.float32, device=plan.device)
        plan.keep.append(shuffled)
        plan.conv(ops.conv_params(wts, src, H, Wd, out_nchw=shuffled, pixel_shuffle=2))
        return shuffled

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        Hp, Wp = h0 + (8 - h0 % 8) % 8, w0 + (8 - w0 % 8) % 8
        if Hp - h0 >= h0 or Wp - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to a multiple of 8')
        dim = self.dim
        with_lo = products == 3
        cache: dict = {}
        x_pl = plan.planes(n, 1, Hp, Wp, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)  # check_img_size's reflect pad, fused

        H1, W1, H2, W2, H3, W3 = Hp // 2, Wp // 2, Hp // 4, Wp // 4, Hp // 8, Wp // 8
        pd = dim // 8
        cat1 = plan.planes(n, 4 * pd, H1, W1, with_lo)  # [dec0's upsampled output (2 dim) | enc1 (2 dim)]
        cat0 = plan.planes(n, 8 * pd, H2, W2, with_lo)  # [the latent stage's upsampled output (4 dim) | enc2 (4 dim)]
        # encoder
        s0 = plan.f32map(n, dim, Hp, Wp)
        plan.conv(ops.conv_params(W['in_to_dim'], x_pl, Hp, Wp, out_f32=s0))
        p0 = plan.planes(n, pd, Hp, Wp, with_lo)
        e0 = self._stage(plan, W, 0, n, Hp, Wp, s0, with_lo, cache, p0, out_f32=True)
        s1 = self._down(plan, W['enc1.0.body.0'], p0, 0, n, Hp, Wp, 2 * dim)
        self._stage(plan, W, 1, n, H1, W1, s1, with_lo, cache, cat1, 2 * pd)
        s2 = self._down(plan, W['enc2.0.body.0'], cat1, 2 * pd, n, H1, W1, 4 * dim)
        self._stage(plan, W, 2, n, H2, W2, s2, with_lo, cache, cat0, 4 * pd)
        # latent
        s3 = self._down(plan, W['latent.0.body.0'], cat0, 4 * pd, n, H2, W2, 8 * dim)
        pl3 = plan.planes(n, 8 * pd, H3, W3, with_lo)
        self._stage(plan, W, 3, n, H3, W3, s3, with_lo, cache, pl3)
        # decoder
        for j, (up_key, src, hh, ww, cat, lin_key, width) in enumerate((('latent.2.body.0', pl3, H3, W3, cat0, 'dec0.0', 4 * dim),
                                                                        ('dec0.2.body.0', None, H2, W2, cat1, 'dec1.0', 2 * dim))):  # fmt: skip
            if src is None:
                src = prev
            shuffled = self._up(plan, W[up_key], src, n, hh, ww, 2 * width)
            half = _view(cat, 0, width // 8)
            plan.call(lambda s=shuffled, dst=half: ops.nchw_to_planes(s, dst))
            plan.count_launches(1)
            sd_ = plan.f32map(n, width, 2 * hh, 2 * ww)
            plan.conv(ops.conv_params(W[lin_key], cat, 2 * hh, 2 * ww, out_f32=sd_))
            prev = plan.planes(n, width // 8, 2 * hh, 2 * ww, with_lo)
            self._stage(plan, W, 4 + j, n, 2 * hh, 2 * ww, sd_, with_lo, cache, prev)
        shuffled = self._up(plan, W['dec1.2.body.0'], prev, n, H1, W1, 2 * dim)
        sc = plan.f32map(n, 2 * dim, Hp, Wp)
        plan.launch('rsa_f32map_concat', dict(a_nchw=shuffled, Ca=dim, b_map=e0, Cb=dim, batch=n, H=Hp, W=Wp, out_map=sc),
                    meta=dict(kernel='rsa_f32map_concat', flop=0, bytes=n * Hp * Wp * 4 * 4 * dim))  # fmt: skip
        p2 = plan.planes(n, 2 * pd, Hp, Wp, with_lo)
        self._stage(plan, W, 6, n, Hp, Wp, sc, with_lo, cache, p2)
        t = plan.planes(n, pd, Hp, Wp, with_lo)
        plan.conv(ops.conv_params(W['dim_to_ch.0'], p2, Hp, Wp, out=t))
        y = plan.output((n, self.in_ch, Hp, Wp), dtype, crop=(h0, w0))
        plan.conv(ops.conv_params(W['dim_to_ch.1'], t, Hp, Wp, out_nchw=y))
        bp = L.BilinearAddParams()  # + the (reflect-padded) input over the region that is kept: scale 1, every weight exactly 0 or 1
        bp.batch, bp.C, bp.h, bp.w, bp.pad_h, bp.pad_w, bp.scale = n, self.in_ch, h0, w0, Hp, Wp, 1
        bp.dtype = ops.rsa_dtype(dtype)
        bp.out_H, bp.out_W, bp.out_h, bp.out_w = Hp, Wp, h0, w0
        bp.x, bp.out = plan.input_ref(x_shape, dtype).data_ptr(), y.data_ptr()
        plan.launch('rsa_bilinear_add', bp)
        return set_input
