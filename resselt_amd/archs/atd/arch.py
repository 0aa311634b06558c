"""ATD (Adaptive Token Dictionary) on the MI355X engine -- drop-in for ``resselt/archs/atd/arch.py:829-1137`` in eval mode.

Tokens are pixels of the flip-padded map.  The residual stream is an f32 map and every Linear layer is a k1 launch of the convolution
kernels.  One ATDTransformerLayer (arch.py:431-489):

  norm1                      rsa_layernorm -> split planes (for wqkv) and an f32 map (for the similarity path)
  wqkv                       k1 convolution into head-grouped planes (head h = planes [h*hp, h*hp + hp), hp = ceil(head_dim / 8))
  ATD_CA     (:223-249)      rsa_atd_dict (k^, V^T of the per-image dictionary) + rsa_atd_ca: sim, category ids, x_atd; f32 similarity path
  AC_MSA     (:289-334)      rsa_atd_sort (stable: ascending token index inside a category) + rsa_atd_attention in category mode
  SW-MSA     (:446-472)      rsa_atd_attention in window mode (roll, partition, bias and shift mask by arithmetic)
  combine    (:474)          one k1 launch over [o_win | o_aca] with the two projections side by side, + shortcut + x_atd
  ConvFFN    (:81-85)        norm2, fc1 + GELU, rsa_atd_dwconv (h + GELU(dw5x5(h))), fc2 + residual
  refinement (:483-487)      rsa_atd_refine on the f32 sim map the layer stored (all but the last layer of a block)

The reference sorts with ``stable=False``, whose order is not defined; the engine defines it as the stable order.  Two debug hooks make the
category path observable: ``atd_record`` (per layer, the ids and permutations used) and ``atd_force`` (permutations to use instead).
"""

from __future__ import annotations

import math

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.transformer import (LayerPacker, ResidualTail, head_macs, head_shapes, layernorm_on, pack_head, reconstruction_head, regroup_proj, regroup_qkv,
                                   relative_position_index, tail_layers, tail_macs, tail_shapes)
from ..dat.arch import pad_rows

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # arch.py:894
MAX_C, MAX_TOKENS, MAX_RC, MAX_HEAD_DIM, MAX_WINDOW, MAX_GROUP = 256, 128, 16, 64, 16, 256  # limits of csrc/atd.hip


def head_planes(embed_dim: int, heads: int) -> int:
    """8-channel planes one head occupies in the qkv / attention-output planes."""
    return (embed_dim // heads + 7) // 8


def atd_param_shapes(in_chans, embed_dim, depths, num_heads, window, num_tokens, reducted_dim, ksize, mlp_ratio, qkv_bias, patch_norm, upscale,
                     upsampler, resi, norm):  # fmt: skip
    s = ParamShapes()
    buffers: dict = {}
    C_ = embed_dim
    hidden = int(C_ * mlp_ratio)
    if not norm:
        buffers['no_norm'] = torch.zeros(1)

    s.conv('conv_first', C_, in_chans, 3)
    if patch_norm:
        s.norm('patch_embed.norm', C_)
    buffers['relative_position_index_SA'] = relative_position_index(window)
    for i, depth in enumerate(depths):
        g = f'layers.{i}.residual_group'
        s[f'{g}.td'] = (num_tokens, C_)
        for j in range(depth):
            b = f'{g}.layers.{j}'
            last = j == depth - 1
            if not last:
                s[f'{b}.sigma'] = (num_tokens, 1)
            s.norm(f'{b}.norm1', C_)
            s.norm(f'{b}.norm2', C_)
            if not last:
                s.norm(f'{b}.norm3', num_tokens)
            s.linear(f'{b}.wqkv', 3 * C_, C_, qkv_bias)
            s[f'{b}.attn_win.relative_position_bias_table'] = ((2 * window - 1) ** 2, num_heads[i])
            s.linear(f'{b}.attn_win.proj', C_, C_)
            s[f'{b}.attn_atd.scale'] = (num_tokens,)
            s.linear(f'{b}.attn_atd.wq', reducted_dim, C_, qkv_bias)
            s.linear(f'{b}.attn_atd.wk', reducted_dim, C_, qkv_bias)
            s.linear(f'{b}.attn_atd.wv', C_, C_, qkv_bias)
            s[f'{b}.attn_aca.logit_scale'] = (1, 1)
            s.linear(f'{b}.attn_aca.proj', C_, C_, qkv_bias)
            s.linear(f'{b}.convffn.fc1', hidden, C_)
            s[f'{b}.convffn.dwconv.depthwise_conv.0.weight'] = (hidden, 1, ksize, ksize)
            s[f'{b}.convffn.dwconv.depthwise_conv.0.bias'] = (hidden,)
            s.linear(f'{b}.convffn.fc2', C_, hidden)
        tail_shapes(s, f'layers.{i}.conv', C_, resi)
    s.norm('norm', C_)
    tail_shapes(s, 'conv_after_body', C_, resi)
    head_shapes(s, upsampler, C_, 64, in_chans, upscale)  # ('nearest+conv' is x4 only: ATD.__init__)
    return s, buffers


class ATD(EngineModule):
    hyperparameters = {}
    precisions = ('bf16x3', 'bf16')

    def __init__(self, *, img_size=64, patch_size=1, in_chans=3, embed_dim=90, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=8,
                 category_size=256, num_tokens=64, reducted_dim=4, convffn_kernel_size=5, mlp_ratio=2.0, qkv_bias=True, norm_layer=None, ape=False,
                 patch_norm=True, upscale=1, img_range=1.0, upsampler='', resi_connection='1conv', norm=True) -> None:  # fmt: skip
        super().__init__()
        depths, num_heads = list(depths), list(num_heads)
        if ape or patch_size != 1:
            raise NotImplementedError('ATD engine supports patch_size=1 and ape=False (what released checkpoints use)')
        if not 2 <= window_size <= MAX_WINDOW:
            raise NotImplementedError(f'window_size {window_size}: the group-attention kernel takes windows of 2..{MAX_WINDOW} (at most {MAX_GROUP} tokens)')
        if not 1 <= category_size <= MAX_GROUP:
            raise NotImplementedError(f'category_size {category_size}: the group-attention kernel takes groups of at most {MAX_GROUP} tokens')
        if embed_dim > MAX_C or embed_dim % 2:
            raise NotImplementedError(f'embed_dim {embed_dim}: the dictionary kernels take even widths up to {MAX_C}')
        if not 1 <= num_tokens <= MAX_TOKENS or not 1 <= reducted_dim <= MAX_RC:
            raise NotImplementedError(f'num_tokens {num_tokens} / reducted_dim {reducted_dim}: the dictionary kernels take at most {MAX_TOKENS} tokens '
                                      f'and a reduced width of at most {MAX_RC}')  # fmt: skip
        if convffn_kernel_size != 5:
            raise NotImplementedError(f'convffn_kernel_size {convffn_kernel_size}: only the 5x5 depthwise convolution is compiled')
        for h in num_heads:
            if embed_dim % h or embed_dim // h > MAX_HEAD_DIM:
                raise NotImplementedError(f'embed_dim {embed_dim} over {h} heads: head_dim must divide embed_dim and be <= {MAX_HEAD_DIM}')
        if upsampler == 'nearest+conv' and upscale != 4:
            raise NotImplementedError('nearest+conv: only x4 (as the reference)')
        if upsampler == 'pixelshuffle' and upscale not in (1, 2, 3, 4, 8):
            raise NotImplementedError(f'upscale {upscale} is not a 2^n / 3 pixel-shuffle head')
        self.in_chans, self.embed_dim, self.depths, self.num_heads = in_chans, embed_dim, depths, num_heads
        self.window_size, self.category_size, self.num_tokens, self.reducted_dim = window_size, category_size, num_tokens, reducted_dim
        self.mlp_ratio, self.hidden, self.qkv_bias, self.patch_norm = mlp_ratio, int(embed_dim * mlp_ratio), qkv_bias, patch_norm
        self.upscale, self.img_range, self.upsampler, self.resi, self.rgb_norm = upscale, img_range, upsampler, resi_connection, norm
        # debug hooks: read at run time by the plan's steps, eager forwards only (not under ``use_graph``)
        self.atd_record: bool = False  # after a forward: ``atd_recorded`` = per layer (ids, perm), device int32 [b, n]
        self.atd_recorded: list = []
        self.atd_force: list | None = None  # per layer, an integer [b, n] permutation used instead of the engine's argmax + sort
        shapes, buffers = atd_param_shapes(in_chans, embed_dim, depths, num_heads, window_size, num_tokens, reducted_dim, convffn_kernel_size, mlp_ratio,
                                           qkv_bias, patch_norm, upscale, upsampler, resi_connection, norm)  # fmt: skip
        build_param_tree(self, shapes, buffers)

    @property
    def is_norm(self) -> bool:
        return self.rgb_norm

    def n_layers(self) -> int:
        return sum(self.depths)

    # ---------------------------------------------------------------- weights
    def pack_layer(self, sd, b: str, heads: int, last: bool) -> dict:
        """The re-laid-out tensors of one layer (pure torch, CPU-testable)."""
        C_, m = self.embed_dim, self.num_tokens
        pad = 8 * head_planes(C_, heads)

        def f32(t):
            return t.to(torch.float32).contiguous()

        def opt(name, rows):
            t = sd.get(name)
            return f32(t) if t is not None else torch.zeros(rows, dtype=torch.float32, device=sd[f'{b}.wqkv.weight'].device)

        out = {}
        out['wqkv'] = regroup_qkv(sd[f'{b}.wqkv.weight'], sd.get(f'{b}.wqkv.bias'), heads, pad=pad, scale_q=False)
        # x_win + x_aca = [o_win | o_aca] [W_win | W_aca]^T + (b_win + b_aca): one K = 2 * heads * pad Linear
        wp = torch.cat([regroup_proj(sd[f'{b}.attn_win.proj.weight'], heads, pad), regroup_proj(sd[f'{b}.attn_aca.proj.weight'], heads, pad)], dim=1)
        out['proj'] = (wp, f32(sd[f'{b}.attn_win.proj.bias']) + opt(f'{b}.attn_aca.proj.bias', C_))
        out['bias_table'] = f32(sd[f'{b}.attn_win.relative_position_bias_table']).t().contiguous()  # [heads][(2w-1)^2]
        out['wq'], out['bq'] = f32(sd[f'{b}.attn_atd.wq.weight']), opt(f'{b}.attn_atd.wq.bias', self.reducted_dim)
        out['wk'], out['bk'] = f32(sd[f'{b}.attn_atd.wk.weight']), opt(f'{b}.attn_atd.wk.bias', self.reducted_dim)
        out['wv'], out['bv'] = f32(sd[f'{b}.attn_atd.wv.weight']), opt(f'{b}.attn_atd.wv.bias', C_)
        out['ca_scale'] = 1.0 + torch.clamp(f32(sd[f'{b}.attn_atd.scale']), 0, 1) * math.log(m)  # arch.py:242-243
        out['aca_scale'] = float(torch.clamp(f32(sd[f'{b}.attn_aca.logit_scale']), max=math.log(100.0)).exp().reshape(-1)[0])  # arch.py:322
        P1 = (self.hidden + 7) // 8
        out['dw'] = (pad_rows(f32(sd[f'{b}.convffn.dwconv.depthwise_conv.0.weight']).reshape(self.hidden, 25), P1 * 8),
                     pad_rows(f32(sd[f'{b}.convffn.dwconv.depthwise_conv.0.bias']), P1 * 8))  # fmt: skip
        if not last:
            out['norm3'] = (f32(sd[f'{b}.norm3.weight']), f32(sd[f'{b}.norm3.bias']))
            out['sigma'] = f32(sd[f'{b}.sigma']).reshape(-1).contiguous()
        return out

    def _pack(self, device, products):
        sd = {k: v.detach().to(device) for k, v in self.state_dict().items()}
        pk = LayerPacker(sd, device, products, lambda name: (int(products), products.fmt))
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln

        def resi_conv(name):
            for layer in tail_layers(name, self.resi):
                conv(layer)

        conv('conv_first')
        if self.patch_norm:
            ln('patch_embed.norm')
        for i, depth in enumerate(self.depths):
            heads = self.num_heads[i]
            g = f'layers.{i}.residual_group'
            W[f'{g}.td'] = sd[f'{g}.td'].to(torch.float32).contiguous()
            for j in range(depth):
                b = f'{g}.layers.{j}'
                ln(f'{b}.norm1')
                ln(f'{b}.norm2')
                t = self.pack_layer(sd, b, heads, j == depth - 1)
                lin(f'{b}.wqkv', *t.pop('wqkv'))
                lin(f'{b}.proj', *t.pop('proj'), cin_planes=2 * heads * head_planes(self.embed_dim, heads))
                lin(f'{b}.convffn.fc1')
                lin(f'{b}.convffn.fc2')
                W[f'{b}.t'] = t
            resi_conv(f'layers.{i}.conv')
        ln('norm')
        resi_conv('conv_after_body')
        pack_head(pk)
        check_fp16_range(v for v in W.values() if isinstance(v, ops.ConvWeights))
        W['mean'] = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=device)
        return W

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per (padded) input pixel: convolutions, Linear layers, the three attentions and the refinement."""
        C_, hid, m, rc, w = self.embed_dim, self.hidden, self.num_tokens, self.reducted_dim, self.window_size
        macs = 9 * self.in_chans * C_
        resi = tail_macs(C_, self.resi)
        for d in self.depths:
            layer = 3 * C_ * C_ + 2 * C_ * C_ + rc * C_ + m * rc + m * C_ + 2 * w * w * C_ + 2 * self.category_size * C_ + 2 * C_ * hid + 25 * hid
            macs += d * layer + (d - 1) * m * C_ + resi
        return macs + resi + head_macs(self.upsampler, C_, 64, self.in_chans, self.upscale)

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, h0, w0 = x_shape
        if c != self.in_chans:
            raise RuntimeError(f'model expects {self.in_chans} input channels, got {c}')
        win = self.window_size
        H, Wd = h0 + (win - h0 % win) % win, w0 + (win - w0 % win) % win
        if 2 * h0 < H or 2 * w0 < Wd:
            # the flip padding (arch.py:1090-1096) appends ONE mirrored copy: a side below half a window stays short of the window multiple,
            # and the reference's window partition fails on it; from half a window on (4..7 for a window of 8) the reference runs
            raise RuntimeError(f'a {h0}x{w0} input is below half a {win}x{win} window: one flip cannot pad it to {H}x{Wd}')
        C_, s, m, rc, hidden = self.embed_dim, self.upscale, self.num_tokens, self.reducted_dim, self.hidden
        ntok = H * Wd
        gs = min(ntok, self.category_size)
        with_lo = products == 3
        prod = int(products)
        cp = (C_ + 7) // 8
        P1 = (hidden + 7) // 8
        Cp32 = (C_ + 31) // 32 * 32
        dev = plan.device
        lib = L.load()
        model = self

        x_pl = plan.planes(n, (c + 7) // 8, H, Wd, with_lo)
        mean = W['mean']
        sub_mean = mean if self.rgb_norm else None
        in_scale = self.img_range if self.rgb_norm else 1.0

        def set_input(x):
            # flip padding to the window multiple (arch.py:1090-1096), then (x - mean) * img_range fused into the layout kernel
            if H != h0:
                x = torch.cat([x, torch.flip(x, [2])], 2)[:, :, :H, :]
            if Wd != w0:
                x = torch.cat([x, torch.flip(x, [3])], 3)[:, :, :, :Wd]
            ops.nchw_to_planes(x.contiguous(), x_pl, sub_mean, in_scale)

        def i32(*shape):
            t = torch.empty(shape, dtype=torch.int32, device=dev)
            plan.keep.append(t)
            return t

        def f32buf(*shape):
            t = torch.empty(shape, dtype=torch.float32, device=dev)
            plan.keep.append(t)
            return t

        first = plan.f32map(n, C_, H, Wd)
        pool = [plan.f32map(n, C_, H, Wd) for _ in range(4)]
        xn_f32 = plan.f32map(n, C_, H, Wd)
        xatd = plan.f32map(n, C_, H, Wd)
        a_pl = plan.planes(n, cp, H, Wd, with_lo)
        max_hp = max(h * head_planes(C_, h) for h in self.num_heads)
        qkv_pl = plan.planes(n, 3 * max_hp, H, Wd, with_lo)
        cat_pl = plan.planes(n, 2 * max_hp, H, Wd, with_lo)  # o_win | o_aca
        hid_pl = plan.planes(n, P1, H, Wd, with_lo)
        hid2_pl = plan.planes(n, P1, H, Wd, with_lo)
        body_pl = plan.planes(n, cp, H, Wd, with_lo)
        resi_conv = ResidualTail(plan, W, self.resi, n, H, Wd, C_, with_lo)
        td_buf = f32buf(n, m, C_)
        kn = f32buf(n, m, 16)
        vt_hi = torch.empty((n, Cp32, 128), dtype=torch.bfloat16, device=dev)
        vt_lo = torch.empty_like(vt_hi)
        plan.keep += [vt_hi, vt_lo]
        sim = f32buf(n, ntok, m)  # f32: the refinement normalises it over all pixels (stored, not recomputed)
        ids, perm, inv = i32(n, ntok), i32(n, ntok), i32(n, ntok)
        sort_ws = torch.empty(max(int(lib.rsa_atd_sort_workspace_bytes(n, ntok)), 16), dtype=torch.uint8, device=dev)
        refine_ws = torch.empty(max(int(lib.rsa_atd_refine_workspace_bytes(n, H, Wd, C_, m)), 16), dtype=torch.uint8, device=dev)
        plan.keep += [sort_ws, refine_ws]

        norm = layernorm_on(plan, W, n, H, Wd, C_)

        def dictionary(t):
            dp = L.AtdDictParams()
            dp.batch, dp.C, dp.m, dp.rc = n, C_, m, rc
            dp.td, dp.wk, dp.bk, dp.wv, dp.bv = td_buf.data_ptr(), t['wk'].data_ptr(), t['bk'].data_ptr(), t['wv'].data_ptr(), t['bv'].data_ptr()
            dp.kn, dp.vt_hi, dp.vt_lo = kn.data_ptr(), vt_hi.data_ptr(), vt_lo.data_ptr()
            plan.launch('rsa_atd_dict', dp)

        def cross_attention(t):
            ap = L.AtdCaParams()
            ap.batch, ap.H, ap.W, ap.C, ap.m, ap.rc, ap.products = n, H, Wd, C_, m, rc, prod
            ap.xn, ap.wq, ap.bq, ap.kn, ap.scale = xn_f32.data_ptr(), t['wq'].data_ptr(), t['bq'].data_ptr(), kn.data_ptr(), t['ca_scale'].data_ptr()
            ap.vt_hi, ap.vt_lo = vt_hi.data_ptr(), vt_lo.data_ptr()
            ap.sim, ap.ids, ap.out = sim.data_ptr(), ids.data_ptr(), xatd.data_ptr()
            plan.launch('rsa_atd_ca', ap)

        sort = plan.bound('rsa_atd_sort', dict(ids=ids, batch=n, n=ntok, m=m, perm=perm, inv=inv, workspace=sort_ws))

        def categorise(layer_index):
            def run():
                forced = model.atd_force
                if forced is not None:
                    f = forced[layer_index].to(device=dev).reshape(n, ntok)
                    if int(f.min()) < 0 or int(f.max()) >= ntok:
                        raise ValueError('atd_force: a permutation entry is outside [0, n)')
                    perm.copy_(f.to(torch.int32))
                else:
                    sort()
                if model.atd_record:
                    model.atd_recorded.append((ids.clone(), perm.clone()))

            plan.call(run)
            plan.count_launches(3)

        def attention(heads, mode, shift, scale, bias_table, plane0):
            hp = head_planes(C_, heads)
            ap = L.AtdAttnParams()
            ap.batch, ap.H, ap.W, ap.heads, ap.head_dim, ap.mode = n, H, Wd, heads, C_ // heads, mode
            ap.ws, ap.shift, ap.gs, ap.products, ap.scale = win, shift, gs, prod, scale
            qkv_pl.bind(ap, 'qkv')
            ap.bias_table = None if bias_table is None else bias_table.data_ptr()
            ap.perm = perm.data_ptr() if mode == 1 else None
            cat_pl.bind(ap, 'out', plane0)
            tokens = n * ntok
            G = win * win if mode == 0 else gs
            meta = dict(kernel=f'rsa::atd_attention_kernel ({"window" if mode == 0 else "category"})', products=prod, flop=4.0 * tokens * G * C_,
                        bytes=tokens * heads * hp * 16.0 * 4 * (2 if with_lo else 1))  # fmt: skip
            plan.launch('rsa_atd_attention', ap, meta=meta)

        def dwconv(t):
            dp = L.AtdDwConvParams()
            dp.batch, dp.H, dp.W, dp.planes = n, H, Wd, P1
            hid_pl.bind(dp, 'in')
            dp.weight, dp.bias = t['dw'][0].data_ptr(), t['dw'][1].data_ptr()
            hid2_pl.bind(dp, 'out')
            plan.launch('rsa_atd_dwconv', dp)

        def refine(t, x_f32):
            rp = L.AtdRefineParams()
            rp.batch, rp.H, rp.W, rp.C, rp.m, rp.eps = n, H, Wd, C_, m, 1e-5
            rp.sim, rp.x, rp.gamma, rp.beta, rp.sigma = sim.data_ptr(), x_f32.data_ptr(), t['norm3'][0].data_ptr(), t['norm3'][1].data_ptr(), t['sigma'].data_ptr()
            rp.td, rp.workspace = td_buf.data_ptr(), refine_ws.data_ptr()
            plan.launch('rsa_atd_refine', rp, kernels=4)

        plan.call(lambda: model.atd_recorded.clear())
        plan.conv(ops.conv_params(W['conv_first'], x_pl, H, Wd, out_f32=first))
        free = list(pool)
        if self.patch_norm:
            cur = free.pop()
            norm('patch_embed.norm', first, out_f32=cur)
        else:
            cur = first
        layer_index = 0
        for i, depth in enumerate(self.depths):
            heads = self.num_heads[i]
            hp_all = heads * head_planes(C_, heads)
            g = f'layers.{i}.residual_group'
            group_in = cur
            td0 = W[f'{g}.td']
            plan.call(lambda td0=td0: td_buf.copy_(td0.unsqueeze(0).expand(n, -1, -1)))  # td = self.td.repeat([b, 1, 1]) (arch.py:611)
            plan.count_launches(1)
            for j in range(depth):
                b = f'{g}.layers.{j}'
                t = W[f'{b}.t']
                last = j == depth - 1
                norm(f'{b}.norm1', cur, out_planes=a_pl, out_f32=xn_f32)
                plan.conv(ops.conv_params(W[f'{b}.wqkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                dictionary(t)
                cross_attention(t)
                categorise(layer_index)
                attention(heads, 1, 0, t['aca_scale'], None, hp_all)
                attention(heads, 0, 0 if j % 2 == 0 else win // 2, (C_ // heads) ** -0.5, t['bias_table'], 0)
                x1 = free.pop()
                plan.conv(ops.conv_params(W[f'{b}.proj'], cat_pl, H, Wd, cin_planes=2 * hp_all, res1=cur, alpha=1.0, res2=xatd, beta=1.0, out_f32=x1))
                norm(f'{b}.norm2', x1, out_planes=a_pl)
                plan.conv(ops.conv_params(W[f'{b}.convffn.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
                dwconv(t)
                x2 = free.pop()
                plan.conv(ops.conv_params(W[f'{b}.convffn.fc2'], hid2_pl, H, Wd, cin_planes=P1, res1=x1, alpha=1.0, out_f32=x2,
                                          out=body_pl if last else None))  # fmt: skip
                if not last:
                    refine(t, x2)
                if cur is not group_in and cur is not first:
                    free.append(cur)
                free.append(x1)
                cur = x2
                layer_index += 1
            out = free.pop()
            resi_conv(f'layers.{i}.conv', body_pl, group_in, out_f32=out)
            if group_in is not first:
                free.append(group_in)
            if cur is not group_in:
                free.append(cur)
            cur = out
        norm('norm', cur, out_planes=a_pl)
        resi_conv('conv_after_body', a_pl, first, out_planes=body_pl)  # + conv_first output

        y_out = plan.output((n, self.in_chans, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        # the last store: x / img_range + mean (arch.py:1131-1132)
        reconstruction_head(plan, W, self.upsampler, body_pl, cp, n, H, Wd, s, with_lo, y_out, 1.0 / in_scale, sub_mean, (x_shape, dtype))
        return set_input
