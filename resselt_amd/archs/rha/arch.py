"""RHA ("Residual Hybrid Attention") on the MI355X engine -- drop-in for ``resselt/archs/rha/arch.py:483-565`` in EVAL mode.

The network is to_feat (3x3) -> ``group_blocks`` x GatedGroup -> ``+ x`` -> a UniUpsample v2 head, on the input reflect-padded to a multiple
of ``max(down_list) * window_size``.  A GatedGroup is ``res_blocks`` gated blocks, an OmniShift (one 5x5 depthwise kernel, folded in f64
from its training parameters as the reference does on ``.eval()``: the stored ``conv5x5_reparam`` pair is never read), a 1x1 convolution and
``+ x``.  A GatedCNNBlock (:418-450) is MoSR's (``archs/mosr/arch.py``) with HybridAttention (:398-415) in place of the depthwise
convolution and no ``gamma``; its launch list, with ``C2 = dim / 2``:

  rsa_layernorm (channels-first LayerNorm, eps 1e-6: f32 stream -> planes) -> fc1 3x3 -> [ g | i | c ] plane ranges, c = [ x1 | x2 ]
  -> rsa_rha_window_attn: MaxPool(down) of x2, the cyclic shift, the focused linear attention of every window and the shift back, one
     launch, an f32 map at 1 / down resolution
  -> rsa_rha_mix: [ OmniShift(x1) | bilinear x down of that map ] as ``dim`` channels of planes
  -> aggr 1x1 + Mish (the fused convolution)  -> rsa_rha_gate: mish(g) * cat(i, aggr * c)
  -> fc2 3x3 + Mish + the stream in its epilogue, f32 map out

Block i of a group shifts by 0 (even i) or ``window_size / 2`` (odd i); group g pools by ``down_list[g % len]``.  The residual stream between
blocks stays an f32 map.  The group tail is rsa_dwconv5x5 and a 1x1 convolution whose residual operand is the group's input; the last
group's also adds to_feat's output (``body(x) + x``) and writes the planes the head reads.  The head is ``engine/uniupsample.py``.

The pad multiple, the cyclic roll and the pooled windows span the whole padded input: under tiled ``upscale()`` every tile computes what
the reference computes on that tile.  The caller's input is never written.
"""

from __future__ import annotations

from fractions import Fraction

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16
from ...engine.uniupsample import SAMPLE_MODS, Head, OwnMetaUpsample
from ..mosr.arch import _conv_weights, gate_layout, relayout_gate
from ..rtmosr.arch import fold_omnishift

LN_EPS = 1e-6
HEADS = 8
BUILT_DOWN = (1, 2, 4, 8)
BUILT_WINDOWS = (4, 8)


def omnishift_shapes(shapes: dict, name: str, c: int) -> None:
    for k in (1, 2, 3, 4):
        shapes[f'{name}.alpha{k}'] = (1, c, 1, 1)
    for sub, ks in (('conv1x1', 1), ('conv3x3', 3), ('conv5x5', 5), ('conv5x5_reparam', 5)):
        shapes[f'{name}.{sub}.weight'] = (c, 1, ks, ks)
        shapes[f'{name}.{sub}.bias'] = (c,)


def pack_hybrid(sd, key: str, c2: int, window: int) -> dict:
    """The f32 tensors rsa_rha_window_attn and rsa_rha_mix read for the HybridAttention ``key``: the two Linear weights transposed
    (input-major), the positional encoding transposed to [C2][N], 1 / softplus(scale) in f64, the shared 5x5 filter of the heads and the
    OmniShift of x1 folded in f64 from alpha1..4 / conv1x1 / conv3x3 / conv5x5 (never from ``conv5x5_reparam``)."""
    f32, d64 = torch.float32, torch.float64
    a = f'{key}.att.2'
    n = window * window
    ow, ob = fold_omnishift(sd, f'{key}.conv')
    return dict(
        wqkv_t=sd[f'{a}.qkv.weight'].to(f32).t().contiguous(), bqkv=sd[f'{a}.qkv.bias'].to(f32).contiguous(),
        pos_t=sd[f'{a}.positional_encoding'].to(f32).reshape(n, c2).t().contiguous(),
        isc=(1.0 / torch.nn.functional.softplus(sd[f'{a}.scale'].to(d64).reshape(c2))).to(f32).contiguous(),
        dww=sd[f'{a}.dwc.weight'].to(f32).reshape(c2 // HEADS, 25).contiguous(), dwb=sd[f'{a}.dwc.bias'].to(f32).contiguous(),
        wproj_t=sd[f'{a}.proj.weight'].to(f32).t().contiguous(), bproj=sd[f'{a}.proj.bias'].to(f32).contiguous(), omni_w=ow, omni_b=ob,
    )  # fmt: skip


class RHA(OwnMetaUpsample, EngineModule):  # (the reference's load_state_dict override: arch.py:548-552)
    hyperparameters = {}
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')

    def __init__(self, dim: int = 64, scale: int = 4, in_ch: int = 3, out_ch: int = 3, mid_dim: int = 32, down_list=(8, 4), expansion_ratio: float = 1.5,
                 group_blocks: int = 4, res_blocks: int = 6, upsample: str = 'pixelshuffledirect', unshuffle_mod: bool = False, window_size: int = 8,
                 hidden: int | None = None) -> None:  # fmt: skip
        super().__init__()
        if unshuffle_mod:
            raise NotImplementedError('RHA: unshuffle_mod is not built (the reference cannot load such a checkpoint either: archs/rha/__init__.py)')
        dim, in_ch, out_ch, scale = int(dim), int(in_ch), int(out_ch), int(scale)
        hidden = int(expansion_ratio * dim) if hidden is None else int(hidden)
        down_list = tuple(int(d) for d in down_list)
        if dim % 16 or dim < 16 or dim > 64:
            raise NotImplementedError(f'RHA: dim must be a multiple of 16 from 16 to 64 (dim / 2 fills planes of 8 channels and 8 heads); got {dim}')
        if hidden % 8 or hidden < dim:
            raise NotImplementedError(f'RHA: hidden = int(expansion_ratio * dim) must be a multiple of 8 and at least dim; got {hidden}')
        if window_size not in BUILT_WINDOWS:
            raise NotImplementedError(f'RHA: window_size must be one of {BUILT_WINDOWS}; got {window_size}')
        if not down_list or any(d not in BUILT_DOWN for d in down_list):
            raise NotImplementedError(f'RHA: every entry of down_list must be one of {BUILT_DOWN}; got {list(down_list)}')
        if in_ch < 1 or in_ch > 8:
            raise NotImplementedError(f'RHA: 1 to 8 input channels are built (got {in_ch})')
        if upsample not in SAMPLE_MODS:
            raise NotImplementedError(f'RHA: the head must be one of {SAMPLE_MODS}; got {upsample!r}')
        if group_blocks < 1 or res_blocks < 1:
            raise NotImplementedError(f'RHA: at least one group of at least one block (got {group_blocks} x {res_blocks})')
        self.dim, self.scale, self.in_ch, self.out_ch, self.mid_dim, self.down_list, self.hidden = dim, scale, in_ch, out_ch, int(mid_dim), down_list, hidden
        self.group_blocks, self.res_blocks, self.head, self.window_size = int(group_blocks), int(res_blocks), upsample, int(window_size)
        self.expansion_ratio = hidden / dim
        self.pad = max(down_list) * self.window_size
        self.up = Head('to_img', upsample, scale, dim, out_ch, self.mid_dim)
        c2 = dim // 2
        shapes: dict = {'to_feat.weight': (dim, in_ch, 3, 3), 'to_feat.bias': (dim,)}
        buffers: dict = {}
        for g in range(self.group_blocks):
            grp = f'body.{g}'
            buffers[f'{grp}.down_sample'] = torch.tensor(self.down(g), dtype=torch.uint8)
            for i in range(self.res_blocks):
                b = f'{grp}.body.{i}'
                shapes[f'{b}.norm.weight'], shapes[f'{b}.norm.bias'] = (dim,), (dim,)
                shapes[f'{b}.fc1.weight'], shapes[f'{b}.fc1.bias'] = (2 * hidden, dim, 3, 3), (2 * hidden,)
                a = f'{b}.conv.att.2'
                shapes[f'{a}.scale'] = (1, 1, c2)
                shapes[f'{a}.positional_encoding'] = (1, self.window_size**2, c2)
                shapes[f'{a}.qkv.weight'], shapes[f'{a}.qkv.bias'] = (3 * c2, c2), (3 * c2,)
                shapes[f'{a}.proj.weight'], shapes[f'{a}.proj.bias'] = (c2, c2), (c2,)
                shapes[f'{a}.dwc.weight'], shapes[f'{a}.dwc.bias'] = (c2 // HEADS, 1, 5, 5), (c2 // HEADS,)
                omnishift_shapes(shapes, f'{b}.conv.conv', c2)
                shapes[f'{b}.conv.aggr.0.weight'], shapes[f'{b}.conv.aggr.0.bias'] = (dim, dim, 1, 1), (dim,)
                shapes[f'{b}.fc2.weight'], shapes[f'{b}.fc2.bias'] = (dim, hidden, 3, 3), (dim,)
            omnishift_shapes(shapes, f'{grp}.body.{self.res_blocks}', dim)
            t = f'{grp}.body.{self.res_blocks + 1}'
            shapes[f'{t}.weight'], shapes[f'{t}.bias'] = (dim, dim, 1, 1), (dim,)
        self.up.shapes(shapes, buffers, whole_planes='RHA')
        build_param_tree(self, shapes, buffers)  # (state_dict lists a module's parameters, then its buffers, then its children, as the reference's)

    def down(self, g: int) -> int:
        return self.down_list[g % len(self.down_list)]

    # ---- accounting ----
    def macs_per_input_pixel(self) -> int:
        """Multiply-accumulates per pixel of the padded input, every term at its own resolution: the attention of a group that pools by
        ``down`` (qkv, the two d x d products per head, the 5x5 of v, proj) runs on 1 / down^2 of the pixels; the head's layers behind an
        upsampling step run on more."""
        d, h, c2 = self.dim, self.hidden, self.dim // 2
        hd = c2 // HEADS
        total = Fraction(9 * self.in_ch * d)
        for g in range(self.group_blocks):
            att = Fraction(3 * c2 * c2 + 2 * c2 * hd + 25 * c2 + c2 * c2, self.down(g) ** 2)
            blk = 9 * d * 2 * h + 25 * c2 + att + d * d + 9 * h * d
            total += self.res_blocks * blk + 25 * d + d * d
        px = 1  # pixels per input pixel at the current layer of the head
        up, s, layers = self.head, self.scale, self.up.layers
        for j, (_, co, ci, k) in enumerate(layers):
            total += px * co * ci * k * k
            if up == 'pixelshuffle' and 0 < j < len(layers) - 1:
                px *= co // ci
            if up == 'nearest+conv' and s != 1 and j < len(layers) - 2:
                px *= 9 if s == 3 else 4
        if self.up.dys_index is not None:
            dd = self.up.dys_dim
            total += 2 * dd * 8 * s * s + s * s * dd * self.out_ch
        return int(total)

    # ---- pack ----
    def _blocks(self):
        for g in range(self.group_blocks):
            for i in range(self.res_blocks):
                yield g, i, f'body.{g}.body.{i}'

    def _gate_groups(self):
        h, d = self.hidden, self.dim
        return [(h - d, (1, 1)), (d, (5, 5))] if h > d else [(d, (5, 5))]

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if v.dtype != torch.uint8}
        f32 = torch.float32
        cw = lambda w, b: ops.ConvWeights.from_oihw(w.to(f32), b.to(f32), products, device=device)  # noqa: E731
        perm, i_planes, _, planes = gate_layout(self._gate_groups())
        W: dict = {'to_feat': cw(sd['to_feat.weight'], sd['to_feat.bias']), 'i_planes': i_planes, 'planes': planes}
        for _, _, b in self._blocks():
            w1, b1, w2 = relayout_gate(sd[f'{b}.fc1.weight'], sd[f'{b}.fc1.bias'], sd[f'{b}.fc2.weight'], perm, planes)
            blk = pack_hybrid(sd, f'{b}.conv', self.dim // 2, self.window_size)
            blk['norm'] = (sd[f'{b}.norm.weight'].contiguous(), sd[f'{b}.norm.bias'].contiguous())
            blk['fc1'], blk['fc2'] = cw(w1, b1), cw(w2, sd[f'{b}.fc2.bias'])
            blk['aggr'] = cw(sd[f'{b}.conv.aggr.0.weight'], sd[f'{b}.conv.aggr.0.bias'])
            W[b] = blk
        for g in range(self.group_blocks):
            t = f'body.{g}.body'
            ow, ob = fold_omnishift(sd, f'{t}.{self.res_blocks}')
            W[f'{t}.tail'] = dict(omni_w=ow, omni_b=ob, conv=cw(sd[f'{t}.{self.res_blocks + 1}.weight'], sd[f'{t}.{self.res_blocks + 1}.bias']))
        self.up.pack(W, sd, products, device)
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    # ---- plan ----
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        pad = self.pad
        H, Wd = h0 + (pad - h0 % pad) % pad, w0 + (pad - w0 % pad) % pad
        if H - h0 >= h0 or Wd - w0 >= w0:
            raise RuntimeError(f'input is too small for reflect padding to a multiple of {pad}')
        dim, hidden, ws, s = self.dim, self.hidden, self.window_size, self.scale
        c2, pd, hp, ip = dim // 2, dim // 8, W['planes'], W['i_planes']
        p2 = c2 // 8
        c0 = hp + ip  # c's first plane in the fc1 buffer: [g | i | c], c = [x1 | x2]
        with_lo = products == 3
        px = n * H * Wd
        unit = 16 * (2 if with_lo else 1)

        x_pl = plan.planes(n, 1, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)  # check_img_size's reflect pad, fused

        top, ga, gb, sa, sb = (plan.f32map(n, dim, H, Wd) for _ in range(5))
        N_pl = plan.planes(n, pd, H, Wd, with_lo)
        F_pl = plan.planes(n, 2 * hp, H, Wd, with_lo)
        X_pl = plan.planes(n, pd, H, Wd, with_lo)  # [OmniShift(x1) | upsampled attention]
        A_pl = plan.planes(n, pd, H, Wd, with_lo)  # mish(aggr(.))
        M_pl = plan.planes(n, hp, H, Wd, with_lo)  # what fc2 reads
        T_pl = plan.planes(n, pd, H, Wd, with_lo)  # a group's last block, then its OmniShift
        O_pl = plan.planes(n, pd, H, Wd, with_lo)
        fe = plan.planes(n, pd, H, Wd, with_lo)
        att = {d: plan.f32map(n, c2, H // d, Wd // d) for d in sorted({self.down(g) for g in range(self.group_blocks)})}
        fmt = F_pl.fmt
        geo = dict(batch=n, H=H, W=Wd, fmt=fmt)

        plan.conv(ops.conv_params(W['to_feat'], x_pl, H, Wd, out_f32=top))
        gin, gout = top, ga
        for g in range(self.group_blocks):
            down = self.down(g)
            A32 = att[down]
            cur, nxt = gin, sa
            for i in range(self.res_blocks):
                blk = W[f'body.{g}.body.{i}']
                shift = 0 if i % 2 == 0 else ws // 2
                lp = L.LayerNormParams()
                lp.batch, lp.H, lp.W, lp.C, lp.eps = n, H, Wd, dim, LN_EPS
                lp.x_f32, lp.gamma, lp.beta = cur.data_ptr(), blk['norm'][0].data_ptr(), blk['norm'][1].data_ptr()
                N_pl.bind(lp, 'out')
                lp.out_fmt = N_pl.fmt
                plan.launch('rsa_layernorm', lp)
                plan.conv(ops.conv_params(blk['fc1'], N_pl, H, Wd, out=F_pl))

                # byte models: every operand touched once (halo and neighbour re-reads stay on chip); the pooled map is 1 / down^2 of a map
                ppx = px // (down * down)
                hd = c2 // HEADS
                plan.launch('rsa_rha_window_attn', dict(x=(F_pl, c0 + p2), C2=c2, down=down, window=ws, shift=shift, wqkv_t=blk['wqkv_t'], bqkv=blk['bqkv'],
                                                        pos_t=blk['pos_t'], inv_scale=blk['isc'], dwc_w=blk['dww'], dwc_b=blk['dwb'], wproj_t=blk['wproj_t'],
                                                        bproj=blk['bproj'], out=A32, **geo),
                            meta=dict(kernel='rsa_rha_window_attn', flop=2 * ppx * (4 * c2 * c2 + 2 * c2 * hd + 25 * c2), bytes=px * p2 * unit + ppx * c2 * 4))  # fmt: skip
                plan.launch('rsa_rha_mix', dict(x=(F_pl, c0), att=A32, out=X_pl, C2=c2, down=down, weight=blk['omni_w'], bias=blk['omni_b'], **geo),
                            meta=dict(kernel='rsa_rha_mix', flop=2 * px * (25 * c2 + 4 * c2), bytes=px * p2 * unit + ppx * c2 * 4 + px * pd * unit))  # fmt: skip
                plan.conv(ops.conv_params(blk['aggr'], X_pl, H, Wd, act=L.ACT_MISH, out=A_pl))
                plan.launch('rsa_rha_gate', dict(f=F_pl, a=A_pl, out=M_pl, hidden_planes=hp, i_planes=ip, **geo),
                            meta=dict(kernel='rsa_rha_gate', flop=px * (2 * dim + 8 * hidden), bytes=px * unit * (2 * hp + pd + hp)))  # fmt: skip
                if i < self.res_blocks - 1:
                    plan.conv(ops.conv_params(blk['fc2'], M_pl, H, Wd, act=L.ACT_MISH, res1=cur, alpha=1.0, out_f32=nxt))
                    cur, nxt = nxt, (sb if nxt is sa else sa)
                else:
                    plan.conv(ops.conv_params(blk['fc2'], M_pl, H, Wd, act=L.ACT_MISH, res1=cur, alpha=1.0, out=T_pl))
            tail = W[f'body.{g}.body.tail']
            dp = L.DwConvParams()
            dp.batch, dp.H, dp.W, dp.planes, dp.act, dp.fmt = n, H, Wd, pd, L.ACT_NONE, fmt
            T_pl.bind(dp, 'in')
            dp.weight, dp.bias = tail['omni_w'].data_ptr(), tail['omni_b'].data_ptr()
            O_pl.bind(dp, 'out')
            plan.launch('rsa_dwconv5x5', dp)
            if g < self.group_blocks - 1:
                plan.conv(ops.conv_params(tail['conv'], O_pl, H, Wd, res1=gin, alpha=1.0, out_f32=gout))
                gin, gout = gout, (gb if gout is ga else ga)
            else:  # body(x) + x: the last group's tail also adds to_feat's output and writes what the head reads
                fe32 = plan.f32map(n, dim, H, Wd) if self.up.needs_f32_input(W) else None
                plan.conv(ops.conv_params(tail['conv'], O_pl, H, Wd, res1=gin, alpha=1.0, res2=top, beta=1.0, out=fe, out_f32=fe32))
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        self.up.emit(plan, W, fe, fe32, y, with_lo)
        return set_input
