"""FlexNet on the MI355X engine -- drop-in for ``resselt/archs/flexnet/arch.py:437-489``, linear pipeline.  Training-mode and eval-mode
outputs of the reference are identical (its two dropouts have p = 0 and its loader never sets them), so there is no eval-mode caveat.

The network, on the input reflect-padded right and bottom to a multiple of 8: ``short_cut`` (a ConvBlock) and ``in_to_feat`` (3x3) read the
image; the pipeline is a chain of LBlocks; ``to_img`` reads ``cat(pipeline, short_cut)``.  An LBlock (:284-308) is ``n`` TransformerBlocks
and a ConvBlock over ``cat(input, blocks' output)``; a ConvBlock (:43-62) is ``mish(conv3(mish(conv3(x)))) + conv1(x)``.  A TransformerBlock
(:266-281) is

  x = x + gamma1 * proj( softmax(q k^T / sqrt(dim)) v + lepe(v) ),   q | k | v = qkv(OmniShift(RMSNorm(x))),  per 8 x 8 window, ONE head
  x = x + gamma2 * sigmoid(receptance(s)) * value(key_norm(relu(key(s))^2)),   s = OmniShift(RMSNorm(x))

with ``nn.RMSNorm(eps=None)``: eps = 2^-23 for the f32 the reference runs in.  Pack-time folds, all in f64 and rounded once: an OmniShift
becomes ONE bias-free 5x5 depthwise kernel from ``alpha`` / ``conv1x1`` / ``conv3x3`` / ``conv5x5`` (the reference does that on its first
forward; the stored ``conv5x5_reparam`` is never read); ``dim^-0.5`` goes into the q rows and bias of ``qkv``; ``gamma1`` into ``proj``;
``gamma2`` into the rows of ``value`` and, with ``channel_norm``, ``key_norm.weight`` into its columns; ``key`` and ``receptance`` read the
same tensor and are stacked into one 1x1 layer of ``hidden + dim`` outputs.  Nine launches per block, the residual stream an f32 map:

  rsa_flex_norm_shift (stream -> planes) -> qkv 1x1 -> rsa_flex_window_attn -> proj 1x1 + stream (f32 map)
  -> rsa_flex_norm_shift -> [key | receptance] 1x1 -> rsa_flex_sqrelu on the key planes, in place -> value 1x1 -> rsa_flex_gate_add

The last block of an LBlock writes its sum as planes behind the LBlock's input, so the ConvBlock's three convolutions read the
concatenation as one plane range; ``to_img`` reads ``[pipeline | short_cut]`` the same way.  Heads: ``ps`` is one convolution stored
through depth-to-space, ``dys`` the shared DySample head (engine/dysample.py), ``n+c`` a convolution and then the conv -> nearest ->
LeakyReLU(0.2) chain of engine/uniupsample.py.

Nothing pools over the whole image; the windows and the reflect pad are anchored at the origin of whatever tensor the network is given:
under tiled ``upscale()`` every tile computes what the reference computes on that tile.  The caller's input is never written.
"""

from __future__ import annotations

import torch

from ...engine import dysample as dys
from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import build_param_tree
from ...engine.tensors import PF_BF16
from ...engine.uniupsample import Head
from ..mosr.arch import _conv_weights

RMS_EPS = 2.0**-23  # nn.RMSNorm(eps=None): torch.finfo(torch.float32).eps
WINDOW = 8
UPSAMPLERS = ('ps', 'dys', 'n+c')


def fold_omnishift(sd, key: str) -> torch.Tensor:
    """``OmniShift.reparam_5x5`` (arch.py:88-107) in f64: one bias-free depthwise 5x5 kernel [C, 25], f32."""
    d = torch.float64
    F = torch.nn.functional
    a = sd[f'{key}.alpha'].to(d)
    w1 = sd[f'{key}.conv1x1.weight'].to(d)
    w = (a[0] * F.pad(torch.ones_like(w1), (2, 2, 2, 2)) + a[1] * F.pad(w1, (2, 2, 2, 2)) + a[2] * F.pad(sd[f'{key}.conv3x3.weight'].to(d), (1, 1, 1, 1))
         + a[3] * sd[f'{key}.conv5x5.weight'].to(d))  # fmt: skip
    return w.reshape(w.shape[0], 25).to(torch.float32).contiguous()


def fold_block(sd, b: str, dim: int, channel_norm: bool) -> dict:
    """The folded f32 tensors of TransformerBlock ``b``: OIHW weights (and biases) of its four 1x1 layers, the two 5x5 kernels, the two
    RMSNorm weights, and LePE's weights tap-major [9][C] with its bias."""
    d, f = torch.float64, torch.float32
    g1, g2 = sd[f'{b}.gamma1'].to(d), sd[f'{b}.gamma2'].to(d)
    wq, bq = sd[f'{b}.att.qkv.weight'].to(d).clone(), sd[f'{b}.att.qkv.bias'].to(d).clone()
    wq[:dim] *= dim**-0.5
    bq[:dim] *= dim**-0.5
    wv = g2[:, None] * sd[f'{b}.ffn.value.weight'].to(d)
    if channel_norm:
        wv = wv * sd[f'{b}.ffn.key_norm.weight'].to(d)[None, :]
    oihw = lambda w: w.to(f)[:, :, None, None].contiguous()  # noqa: E731
    return dict(
        qkv_w=oihw(wq), qkv_b=bq.to(f), proj_w=oihw(g1[:, None] * sd[f'{b}.att.proj.weight'].to(d)), proj_b=(g1 * sd[f'{b}.att.proj.bias'].to(d)).to(f),
        kr_w=oihw(torch.cat([sd[f'{b}.ffn.key.weight'].to(d), sd[f'{b}.ffn.receptance.weight'].to(d)], 0)), value_w=oihw(wv),
        shift1=fold_omnishift(sd, f'{b}.att.omni_shift'), shift2=fold_omnishift(sd, f'{b}.ffn.omni_shift'),
        rn1=sd[f'{b}.rn1.weight'].to(f).contiguous(), rn2=sd[f'{b}.rn2.weight'].to(f).contiguous(),
        lepe_w=sd[f'{b}.att.get_v.weight'].to(f).reshape(dim, 9).t().contiguous(), lepe_b=sd[f'{b}.att.get_v.bias'].to(f).contiguous(),
    )  # fmt: skip


def nc_head(scale: int, dim: int, out_ch: int) -> Head:
    """InterpolateUpsampler (arch.py:22-40) as UniUpsample's nearest+conv head; at scale 1 it keeps both of its convolutions."""
    up = Head('to_img.1', 'nearest+conv', scale, dim, out_ch, dim)
    if scale == 1:
        up.layers = [(0, dim, dim, 3), (2, out_ch, dim, 3)]
    return up


class FlexNet(EngineModule):
    hyperparameters = {}
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')

    def __init__(self, inp_channels: int = 3, out_channels: int = 3, scale: int = 4, dim: int = 64, num_blocks=(6, 6, 6, 6, 6, 6), window_size: int = 8,
                 hidden_rate: int = 4, channel_norm: bool = False, attn_drop: float = 0.0, proj_drop: float = 0.0, pipeline_type: str = 'linear',
                 upsampler: str = 'ps') -> None:  # fmt: skip
        super().__init__()
        if pipeline_type != 'linear':
            raise NotImplementedError(f'FlexNet: the {pipeline_type!r} pipeline is not built (the meta U-Net runs the block at up to 8 * dim channels); only linear is')
        if int(window_size) != WINDOW:
            raise NotImplementedError(f'FlexNet: window_size must be 8, got {window_size}: the reference cannot run another one either '
                                      '(LMLTVIT.get_lepe hardcodes H = W = 8 and its view raises a shape error)')  # fmt: skip
        dim, scale, in_ch, out_ch, hidden_rate = int(dim), int(scale), int(inp_channels), int(out_channels), int(hidden_rate)
        num_blocks = tuple(int(b) for b in num_blocks)
        if dim % 16 or dim < 16 or dim > 128:
            raise NotImplementedError(f'FlexNet: dim must be a multiple of 16 from 16 to 128 (the window attention runs one head of dim channels); got {dim}')
        if hidden_rate < 1:
            raise NotImplementedError(f'FlexNet: hidden_rate must be at least 1, got {hidden_rate}')
        if in_ch < 1 or in_ch > 8:
            raise NotImplementedError(f'FlexNet: 1 to 8 input channels are built (got {in_ch})')
        if not num_blocks or any(b < 1 for b in num_blocks):
            raise NotImplementedError(f'FlexNet: at least one LBlock of at least one TransformerBlock each (got {list(num_blocks)})')
        if upsampler not in UPSAMPLERS:
            upsampler = 'ps'  # (the reference's constructor falls through to the pixel-shuffle head for any other string)
        if scale < 1 or out_ch < 1:
            raise NotImplementedError(f'FlexNet: scale and out_channels must be positive (got {scale}, {out_ch})')
        if upsampler == 'n+c' and scale & (scale - 1) and scale != 3:
            raise NotImplementedError(f'FlexNet: the n+c head is built for scales 2^n and 3 (the reference does not upsample at all at scale {scale})')
        if upsampler == 'dys' and out_ch > 4:
            raise NotImplementedError(f'FlexNet: the dys head is built for at most 4 output channels (got {out_ch})')
        self.dim, self.scale, self.in_ch, self.out_ch, self.hidden_rate, self.hidden = dim, scale, in_ch, out_ch, hidden_rate, hidden_rate * dim
        self.num_blocks, self.channel_norm, self.upsampler, self.pipeline_type = num_blocks, bool(channel_norm), upsampler, 'linear'  # (window_size: the buffer, as the reference's)
        self.pad = WINDOW
        shapes: dict = {}
        buffers: dict = {'window_size': torch.tensor(WINDOW, dtype=torch.uint8)}
        if upsampler == 'n+c':
            buffers['scale_factor'] = torch.tensor(scale, dtype=torch.uint8)

        def conv(name, co, ci, k):
            shapes[f'{name}.weight'], shapes[f'{name}.bias'] = (co, ci, k, k), (co,)

        def convblock(name, ci, co):
            conv(f'{name}.block.0', co, ci, 3)
            conv(f'{name}.block.2', co, co, 3)
            conv(f'{name}.conv11', co, ci, 1)

        def omnishift(name):
            shapes[f'{name}.alpha'] = (4,)
            for sub, ks in (('conv1x1', 1), ('conv3x3', 3), ('conv5x5', 5), ('conv5x5_reparam', 5)):
                shapes[f'{name}.{sub}.weight'] = (dim, 1, ks, ks)

        convblock('short_cut', in_ch, dim)
        conv('in_to_feat', dim, in_ch, 3)
        for li, nb in enumerate(num_blocks):
            for bi in range(nb):
                b = f'pipeline.att.{li}.t_blocks.{bi}'
                shapes[f'{b}.gamma1'], shapes[f'{b}.gamma2'] = (dim,), (dim,)
                shapes[f'{b}.rn1.weight'], shapes[f'{b}.rn2.weight'] = (dim,), (dim,)
                shapes[f'{b}.att.qkv.weight'], shapes[f'{b}.att.qkv.bias'] = (3 * dim, dim), (3 * dim,)
                shapes[f'{b}.att.proj.weight'], shapes[f'{b}.att.proj.bias'] = (dim, dim), (dim,)
                omnishift(f'{b}.att.omni_shift')
                shapes[f'{b}.att.get_v.weight'], shapes[f'{b}.att.get_v.bias'] = (dim, 1, 3, 3), (dim,)
                shapes[f'{b}.ffn.key.weight'] = (self.hidden, dim)
                omnishift(f'{b}.ffn.omni_shift')
                if self.channel_norm:
                    shapes[f'{b}.ffn.key_norm.weight'] = (self.hidden,)
                shapes[f'{b}.ffn.receptance.weight'] = (dim, dim)
                shapes[f'{b}.ffn.value.weight'] = (dim, self.hidden)
            convblock(f'pipeline.att.{li}.conv', 2 * dim, dim)
        self.layers = []
        if upsampler == 'n+c':
            conv('to_img.0', dim, 2 * dim, 3)
            self.up = nc_head(scale, dim, out_ch)
            self.layers = self.up.layers
            for i, co, ci, k in self.layers:
                conv(f'to_img.1.{i}', co, ci, k)
        elif upsampler == 'dys':
            conv('to_img.end_conv', out_ch, 2 * dim, 1)
            conv('to_img.offset', 8 * scale * scale, 2 * dim, 1)
            shapes['to_img.scope.weight'] = (8 * scale * scale, 2 * dim, 1, 1)
            buffers['to_img.init_pos'] = dys.dysample_init_pos(scale, 4)
        else:
            conv('to_img.0', out_ch * scale * scale, 2 * dim, 3)
        build_param_tree(self, shapes, buffers)  # (state_dict lists a module's parameters, then its buffers, then its children, as the reference's)

    # ---- accounting ----
    def macs_per_input_pixel(self) -> int:
        """Multiply-accumulates per pixel of the padded input; the head's layers behind an upsampling step run on more pixels."""
        d, h, ci, s, o = self.dim, self.hidden, self.in_ch, self.scale, self.out_ch
        block = 25 * d + 3 * d * d + 2 * 64 * d + 9 * d + d * d + 25 * d + (h + d) * d + h * d
        convblock = lambda i: 9 * i * d + 9 * d * d + i * d  # noqa: E731
        total = convblock(ci) + 9 * ci * d + sum(nb * block + convblock(2 * d) for nb in self.num_blocks)
        if self.upsampler == 'ps':
            total += 9 * 2 * d * o * s * s
        elif self.upsampler == 'dys':
            total += 2 * 2 * d * 8 * s * s + 2 * d * 16  # offset and scope; the end convolution, projected per group before the sampling
        else:
            total += 9 * 2 * d * d
            px = 1
            for j, (_, co, cin, k) in enumerate(self.layers):
                total += px * co * cin * k * k
                if s != 1 and j < len(self.layers) - 2:
                    px *= 9 if s == 3 else 4
        return int(total)

    # ---- pack ----
    def _blocks(self):
        for li, nb in enumerate(self.num_blocks):
            for bi in range(nb):
                yield li, bi, f'pipeline.att.{li}.t_blocks.{bi}'

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if v.dtype != torch.uint8}
        cw = lambda w, b: ops.ConvWeights.from_oihw(w.to(torch.float32), None if b is None else b.to(torch.float32), products, device=device)  # noqa: E731

        def convblock(name):
            return dict(b0=cw(sd[f'{name}.block.0.weight'], sd[f'{name}.block.0.bias']), b2=cw(sd[f'{name}.block.2.weight'], sd[f'{name}.block.2.bias']),
                        c11=cw(sd[f'{name}.conv11.weight'], sd[f'{name}.conv11.bias']))  # fmt: skip

        W: dict = {'short_cut': convblock('short_cut'), 'in_to_feat': cw(sd['in_to_feat.weight'], sd['in_to_feat.bias'])}
        for _, _, b in self._blocks():
            f = fold_block(sd, b, self.dim, self.channel_norm)
            W[b] = dict(qkv=cw(f['qkv_w'], f['qkv_b']), proj=cw(f['proj_w'], f['proj_b']), kr=cw(f['kr_w'], None), value=cw(f['value_w'], None),
                        **{k: f[k] for k in ('shift1', 'shift2', 'rn1', 'rn2', 'lepe_w', 'lepe_b')})  # fmt: skip
        for li in range(len(self.num_blocks)):
            W[f'pipeline.att.{li}.conv'] = convblock(f'pipeline.att.{li}.conv')
        if self.upsampler == 'n+c':
            W['to_img.0'] = cw(sd['to_img.0.weight'], sd['to_img.0.bias'])
            self.up.pack(W, sd, products, device)
        elif self.upsampler == 'dys':
            dys.pack(W, sd['to_img.offset.weight'], sd['to_img.offset.bias'], sd['to_img.scope.weight'], sd['to_img.end_conv.weight'].reshape(self.out_ch, -1),
                     sd['to_img.end_conv.bias'], sd['to_img.init_pos'], 4, self.scale, products=products, device=device)  # fmt: skip
        else:
            W['to_img.0'] = cw(sd['to_img.0.weight'], sd['to_img.0.bias'])
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
        dim, hidden, s = self.dim, self.hidden, self.scale
        pd, hp = dim // 8, hidden // 8
        with_lo = products == 3
        prod = int(products)
        px = n * H * Wd
        unit = 16 * (2 if with_lo else 1)
        MISH = L.ACT_MISH

        x_pl = plan.planes(n, 1, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)  # check_img_size's reflect pad, fused

        sa, sb, c11 = (plan.f32map(n, dim, H, Wd) for _ in range(3))
        T_pl = plan.planes(n, pd, H, Wd, with_lo)  # a ConvBlock's first convolution
        SC = plan.planes(n, 2 * pd, H, Wd, with_lo)  # what to_img reads: [pipeline | short_cut]
        CAT = plan.planes(n, 2 * pd, H, Wd, with_lo)  # what an LBlock's ConvBlock reads: [its input | its blocks' output]
        NS = plan.planes(n, pd, H, Wd, with_lo)  # OmniShift(RMSNorm(stream))
        QKV = plan.planes(n, 3 * pd, H, Wd, with_lo)
        A_pl = plan.planes(n, pd, H, Wd, with_lo)  # attention + lepe
        KR = plan.planes(n, hp + pd, H, Wd, with_lo)  # [key | receptance]
        KV = plan.planes(n, pd, H, Wd, with_lo)
        geo = dict(batch=n, H=H, W=Wd, fmt=NS.fmt)

        def convblock(w, src, out, out_plane_off=0, out_f32=None):
            plan.conv(ops.conv_params(w['c11'], src, H, Wd, out_f32=c11))
            plan.conv(ops.conv_params(w['b0'], src, H, Wd, act=MISH, out=T_pl))
            plan.conv(ops.conv_params(w['b2'], T_pl, H, Wd, act=MISH, res1=c11, alpha=1.0, out=out, out_plane_off=out_plane_off, out_f32=out_f32))

        def norm_shift(src, nw, w):
            # bytes: the stream is read twice (once for the norms, once plane by plane: the second pass hits L2), the planes written once
            plan.launch('rsa_flex_norm_shift', dict(x_f32=src, eps=RMS_EPS, norm_weight=nw, weight=w, out=NS, C=dim, **geo),
                        meta=dict(kernel='rsa_flex_norm_shift', flop=px * dim * (2 + 2 + 50), bytes=px * dim * 4 + px * pd * unit))  # fmt: skip

        convblock(W['short_cut'], x_pl, SC, out_plane_off=pd)
        plan.conv(ops.conv_params(W['in_to_feat'], x_pl, H, Wd, out=CAT, out_f32=sa))
        last_l = len(self.num_blocks) - 1
        for li, nb in enumerate(self.num_blocks):
            for bi in range(nb):
                blk = W[f'pipeline.att.{li}.t_blocks.{bi}']
                norm_shift(sa, blk['rn1'], blk['shift1'])
                plan.conv(ops.conv_params(blk['qkv'], NS, H, Wd, out=QKV))
                plan.launch('rsa_flex_window_attn', dict(qkv=QKV, out=A_pl, C=dim, products=prod, lepe_w=blk['lepe_w'], lepe_b=blk['lepe_b'], **geo),
                            meta=dict(kernel='rsa_flex_window_attn', flop=2 * px * (2 * 64 * dim + 9 * dim), bytes=px * (3 * pd + pd) * unit))  # fmt: skip
                plan.conv(ops.conv_params(blk['proj'], A_pl, H, Wd, res1=sa, alpha=1.0, out_f32=sb))
                norm_shift(sb, blk['rn2'], blk['shift2'])
                plan.conv(ops.conv_params(blk['kr'], NS, H, Wd, out=KR))
                plan.launch('rsa_flex_sqrelu', dict(in_=KR, out=KR, hidden=hidden, norm=1 if self.channel_norm else 0, eps=RMS_EPS, **geo),
                            meta=dict(kernel='rsa_flex_sqrelu', flop=px * hidden * (4 if self.channel_norm else 2), bytes=2 * px * hp * unit))  # fmt: skip
                plan.conv(ops.conv_params(blk['value'], KR, H, Wd, in_plane0=0, cin_planes=hp, out=KV))
                last = bi == nb - 1
                # a block's last gate writes the planes the LBlock's ConvBlock reads; the others write the f32 stream
                out = dict(out=(CAT, pd), out_f32=None) if last else dict(out_hi=None, out_lo=None, out_plane_stride=CAT.plane_stride, out_batch_stride=CAT.batch_stride, out_f32=sa)
                plan.launch('rsa_flex_gate_add', dict(r=(KR, hp), kv=KV, base_f32=sb, C=dim, **out, **geo),
                            meta=dict(kernel='rsa_flex_gate_add', flop=px * dim * 4, bytes=px * (2 * pd * unit + dim * 4 + (pd * unit if last else dim * 4))))  # fmt: skip
            w = W[f'pipeline.att.{li}.conv']
            if li < last_l:
                convblock(w, CAT, CAT, out_f32=sa)  # (the third convolution reads T_pl: CAT's first half is free by then)
            else:
                convblock(w, CAT, SC)
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        if self.upsampler == 'ps':
            plan.conv(ops.conv_params(W['to_img.0'], SC, H, Wd, out_nchw=y, pixel_shuffle=s))
        elif self.upsampler == 'dys':
            dys.emit(plan, W, SC, y, None)
        else:
            fe = plan.planes(n, pd, H, Wd, with_lo)
            plan.conv(ops.conv_params(W['to_img.0'], SC, H, Wd, out=fe))
            if s == 1:
                o = plan.planes(n, pd, H, Wd, with_lo)
                plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.2, out=o))
                plan.conv(ops.conv_params(W['head1'], o, H, Wd, out_nchw=y))
            else:
                self.up.emit(plan, W, fe, None, y, with_lo)
        return set_input
