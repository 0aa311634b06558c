"""RGT (Recursive Generalization Transformer) on the MI355X engine -- drop-in for ``resselt/archs/rgt/arch.py:630-838`` in eval mode.

Tokens are pixels.  The residual stream is an f32 map and every Linear layer is a k1 launch of the convolution kernels.  Blocks alternate:

  L_SA  (even blocks, arch.py:370-447)  LN -> qkv -> 2 x rect-window attention (DAT's rsa_rect_attention: the split and its transpose on
                                        the two channel halves, shifted by DAT's rule) -> + depthwise conv(v) -> proj (+ residual)
  RG_SA (odd blocks,  arch.py:500-544)  LN -> q on every token; the same LN output reduced t times by the 4x4 stride-4 `reduction1`
                                        (rsa_rg_reduce) -> dwconv -> 1x1 -> LN + GELU -> k, v -> v + cpe(v) on the pooled map (at most
                                        63 x 63 tokens) -> rsa_rg_attention: every token against all pooled tokens -> proj (+ residual)
  MLP   (arch.py:37-84)                 DAT's SGFN: LN -> fc1 + GELU -> x1 * dwconv(LN(x2)) -> fc2 (+ residual)
  HAI   (arch.py:612-619)               x + gamma * (block input): rsa_scale_add on the post-attention stream once norm2 has read it

Attention-side maps use the head-padded layout (head h = channels [32h, 32h+32)); the L_SA proj reads the attention output and the
depthwise conv of v side by side (planes [0, 4*heads) and [4*heads, 8*heads)) with its weights repeated, which is the sum
``attened_x + lcm`` of arch.py:441.  The recursion count t is computed per input size on the host, with the reference's expression.
"""

from __future__ import annotations

import math

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.transformer import (HEAD_PAD, LayerPacker, ResidualTail, bias_fragments_qk, branch_geometry, dwconv3x3, head_shapes, layernorm_on, pack_head,
                                   pad_heads, pixelshuffle_macs, plane_stats, reconstruction_head, rect_attention, regroup_proj, regroup_qkv, tail_layers,
                                   tail_macs, tail_shapes)
from ..dat.arch import is_shifted, pad_rows, rpe_buffers, shift_masks

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # arch.py:656
RG_MAX_KEYS = 63 * 63  # RSA_RG_MAX_KEYS


def rg_times(H: int, W: int) -> int:
    """RG_SA's eval recursion count (arch.py:516-519), verbatim: raises ValueError (math domain error) when H < 16 or W < 16."""
    t = max(int(math.log(H // 16, 4)), int(math.log(W // 16, 4)))
    return max(t, 2)


def rg_scale(embed_dim: int, heads: int, c_ratio: float) -> float:
    """RG_SA.scale (arch.py:488): (head_dim * c_ratio) ** -0.5 with head_dim = dim // heads."""
    return (embed_dim // heads * c_ratio) ** -0.5


def rgt_param_shapes(in_chans, embed_dim, split_size, depth, num_heads, mlp_ratio, qkv_bias, upscale, resi, c_ratio, img_size):
    s = ParamShapes()
    buffers: dict = {}
    C_ = embed_dim
    hidden = int(C_ * mlp_ratio)
    cr = int(C_ * c_ratio)
    shift_size = [split_size[0] // 2, split_size[1] // 2]
    pos_dim = ((C_ // 2) // 4) // 4

    def dw(name, c, k=3):
        s[f'{name}.weight'] = (c, 1, k, k)
        s[f'{name}.bias'] = (c,)

    s.conv('conv_first', C_, in_chans, 3)
    s.norm('before_RG.1', C_)
    masks = None
    for i, d in enumerate(depth):
        heads = num_heads[i]
        for j in range(d):
            b = f'layers.{i}.blocks.{j}'
            s.norm(f'{b}.norm1', C_)
            if j % 2 == 0:
                s.linear(f'{b}.attn.qkv', 3 * C_, C_, qkv_bias)
                s.linear(f'{b}.attn.proj', C_, C_)
                for idx in (0, 1):
                    a = f'{b}.attn.attns.{idx}'
                    hs, ws = branch_geometry(split_size, idx)
                    buffers[f'{a}.rpe_biases'], buffers[f'{a}.relative_position_index'] = rpe_buffers(hs, ws)
                    s.linear(f'{a}.pos.pos_proj', pos_dim, 2)
                    for k, co in (('pos1', pos_dim), ('pos2', pos_dim), ('pos3', heads // 2)):
                        s.norm(f'{a}.pos.{k}.0', pos_dim)
                        s.linear(f'{a}.pos.{k}.2', co, pos_dim)
                if is_shifted(i, j):
                    if masks is None:
                        masks = shift_masks(img_size, img_size, split_size, shift_size)
                    buffers[f'{b}.attn.attn_mask_0'], buffers[f'{b}.attn.attn_mask_1'] = masks
                dw(f'{b}.attn.get_v', C_)
            else:
                dw(f'{b}.attn.reduction1', C_, 4)
                dw(f'{b}.attn.dwconv', C_)
                s.conv(f'{b}.attn.conv', cr, C_, 1)
                s.norm(f'{b}.attn.norm_act.0', cr)
                s.linear(f'{b}.attn.q', cr, C_, qkv_bias)
                s.linear(f'{b}.attn.k', cr, cr, qkv_bias)
                s.linear(f'{b}.attn.v', C_, cr, qkv_bias)
                dw(f'{b}.attn.cpe', C_)
                s.linear(f'{b}.attn.proj', C_, C_)
            s.linear(f'{b}.mlp.fc1', hidden, C_)
            s.norm(f'{b}.mlp.sg.norm', hidden // 2)
            dw(f'{b}.mlp.sg.conv', hidden // 2)
            s.linear(f'{b}.mlp.fc2', C_, hidden // 2)
            s.norm(f'{b}.norm2', C_)
            s[f'{b}.gamma'] = (C_,)
        tail_shapes(s, f'layers.{i}.conv', C_, resi)
    s.norm('norm', C_)
    tail_shapes(s, 'conv_after_body', C_, resi)
    head_shapes(s, 'pixelshuffle', C_, 64, in_chans, upscale)
    return s, buffers


class RGT(EngineModule):
    hyperparameters = {}
    precisions = ('bf16x3', 'bf16')

    def __init__(self, *, img_size=64, in_chans=3, embed_dim=180, depth=(2, 2, 2, 2), num_heads=(2, 2, 2, 2), mlp_ratio=4.0, qkv_bias=True,
                 qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_chk=False, upscale=2, img_range=1.0,
                 resi_connection='1conv', split_size=(8, 8), c_ratio=0.5) -> None:  # fmt: skip
        super().__init__()
        split_size, depth, num_heads = list(split_size), list(depth), list(num_heads)
        if qk_scale is not None:
            raise NotImplementedError('RGT engine supports the default qk scale (what the loader builds)')
        if upscale not in (1, 2, 3, 4, 8):
            raise NotImplementedError(f'upscale {upscale} is not a 2^n / 3 pixel-shuffle head')
        if split_size[0] * split_size[1] > 256 or min(split_size) < 2:
            raise NotImplementedError('split_size must hold 4..256 tokens with both sides >= 2')
        if embed_dim % 4:
            raise NotImplementedError('embed_dim must be a multiple of 4')
        cr = int(embed_dim * c_ratio)
        for h in num_heads:
            if h % 2:
                raise NotImplementedError(f'{h} heads: the L_SA branches need an even head count (each branch runs heads // 2)')
            if embed_dim % h or embed_dim // h > HEAD_PAD:
                raise NotImplementedError(f'embed_dim {embed_dim} over {h} heads: head_dim must divide embed_dim and be <= {HEAD_PAD}')
            if any(d >= 2 for d in depth) and (cr % h or cr // h > HEAD_PAD or cr < 1):
                raise NotImplementedError(f'RG-SA q/k width {cr} over {h} heads: the per-head width must divide it and be <= {HEAD_PAD}')
        hidden = int(embed_dim * mlp_ratio)
        if hidden % 2:
            raise NotImplementedError('the MLP hidden width must be even')
        self.in_chans, self.embed_dim, self.split_size, self.depth, self.num_heads = in_chans, embed_dim, split_size, depth, num_heads
        self.hidden, self.qkv_bias, self.upscale, self.img_range = hidden, qkv_bias, upscale, img_range
        self.resi, self.c_ratio, self.cr, self.img_size = resi_connection, c_ratio, cr, img_size
        shapes, buffers = rgt_param_shapes(in_chans, embed_dim, split_size, depth, num_heads, mlp_ratio, qkv_bias, upscale, resi_connection, c_ratio,
                                           img_size)  # fmt: skip
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device) for k, v in self.state_dict().items()}
        C_, cr = self.embed_dim, self.cr
        cp = (C_ + 7) // 8
        pk = LayerPacker(sd, device, products, lambda name: (int(products), products.fmt))
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln

        def f32(t):
            return t.to(torch.float32).contiguous()

        def resi_conv(name):
            for layer in tail_layers(name, self.resi):
                conv(layer)

        def pos_bias(a):
            """DynamicPosBias (residual=False, arch.py:94-118) on rpe_biases, gathered to [heads, N, N] (arch.py:218-224)."""
            F = torch.nn.functional
            pos = F.linear(f32(sd[f'{a}.rpe_biases']), f32(sd[f'{a}.pos.pos_proj.weight']), f32(sd[f'{a}.pos.pos_proj.bias']))
            for k in ('pos1', 'pos2', 'pos3'):
                g = f32(sd[f'{a}.pos.{k}.0.weight'])
                pos = F.layer_norm(pos, (g.shape[0],), g, f32(sd[f'{a}.pos.{k}.0.bias']), 1e-5)
                pos = F.linear(F.relu(pos), f32(sd[f'{a}.pos.{k}.2.weight']), f32(sd[f'{a}.pos.{k}.2.bias']))
            idx = sd[f'{a}.relative_position_index'].long()
            n = idx.shape[0]
            return pos[idx.reshape(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()

        def opt_bias(name, rows):
            b = sd.get(f'{name}.bias')
            return f32(b) if b is not None else torch.zeros(rows, dtype=torch.float32, device=device)

        half = self.hidden // 2
        P1 = (half + 7) // 8
        conv('conv_first')
        ln('before_RG.1')
        for i, d in enumerate(self.depth):
            heads = self.num_heads[i]
            for j in range(d):
                b = f'layers.{i}.blocks.{j}'
                a = f'{b}.attn'
                ln(f'{b}.norm1')
                ln(f'{b}.norm2')
                wp = regroup_proj(sd[f'{a}.proj.weight'], heads)
                if j % 2 == 0:
                    wq, bq = regroup_qkv(sd[f'{a}.qkv.weight'], sd.get(f'{a}.qkv.bias'), heads)
                    lin(f'{a}.qkv', wq, bq)
                    # proj(attened_x + get_v(v)): one k1 launch over both halves side by side
                    lin(f'{a}.proj', torch.cat([wp, wp], dim=1), sd[f'{a}.proj.bias'], cin_planes=2 * heads * HEAD_PAD // 8)
                    for idx in (0, 1):
                        W[f'{a}.bias{idx}'] = bias_fragments_qk(pos_bias(f'{a}.attns.{idx}'))
                    W[f'{a}.get_v'] = (pad_heads(f32(sd[f'{a}.get_v.weight']).reshape(C_, 9), heads), pad_heads(f32(sd[f'{a}.get_v.bias']), heads))
                else:
                    W.update(self._pack_rg(sd, a, heads, device))
                    lin(f'{a}.q', *W.pop(f'{a}.q'))
                    lin(f'{a}.kv', *W.pop(f'{a}.kv'))
                    lin(f'{a}.conv', f32(sd[f'{a}.conv.weight']).reshape(cr, C_), f32(sd[f'{a}.conv.bias']))
                    ln(f'{a}.norm_act.0')
                    lin(f'{a}.proj', wp, sd[f'{a}.proj.bias'], cin_planes=heads * HEAD_PAD // 8)
                    W[f'{a}.reduction1'] = (pad_rows(f32(sd[f'{a}.reduction1.weight']).reshape(C_, 16), cp * 8), pad_rows(f32(sd[f'{a}.reduction1.bias']), cp * 8))
                    W[f'{a}.dwconv'] = (pad_rows(f32(sd[f'{a}.dwconv.weight']).reshape(C_, 9), cp * 8), pad_rows(f32(sd[f'{a}.dwconv.bias']), cp * 8))
                # MLP: fc1 rows x1 = [0, half) on planes [0, P1), x2 = [half, 2*half) on planes [P1, 2*P1) (as DAT's SGFN)
                w1 = torch.zeros((2 * P1 * 8, C_), dtype=torch.float32, device=device)
                b1 = torch.zeros((2 * P1 * 8,), dtype=torch.float32, device=device)
                fw, fb = f32(sd[f'{b}.mlp.fc1.weight']), f32(sd[f'{b}.mlp.fc1.bias'])
                w1[:half], w1[P1 * 8 : P1 * 8 + half] = fw[:half], fw[half:]
                b1[:half], b1[P1 * 8 : P1 * 8 + half] = fb[:half], fb[half:]
                lin(f'{b}.mlp.fc1', w1, b1)
                lin(f'{b}.mlp.fc2')
                W[f'{b}.mlp.sg'] = (pad_rows(f32(sd[f'{b}.mlp.sg.conv.weight']).reshape(half, 9), P1 * 8), pad_rows(f32(sd[f'{b}.mlp.sg.conv.bias']), P1 * 8),
                                    pad_rows(f32(sd[f'{b}.mlp.sg.norm.weight']), P1 * 8), pad_rows(f32(sd[f'{b}.mlp.sg.norm.bias']), P1 * 8))  # fmt: skip
                W[f'{b}.gamma'] = f32(sd[f'{b}.gamma'])
            resi_conv(f'layers.{i}.conv')
        ln('norm')
        resi_conv('conv_after_body')
        pack_head(pk)
        check_fp16_range(W.values())
        W['mean'] = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=device)
        return W

    def _pack_rg(self, sd, a, heads, device) -> dict:
        """The re-laid-out tensors of one RG_SA (pure torch, CPU-testable): head-padded q (scale folded) and k | v rows, CPE folded with its
        residual (v + cpe(v) = a depthwise conv whose centre tap is one larger)."""
        C_, cr = self.embed_dim, self.cr
        dq, dv = cr // heads, C_ // heads
        scale = rg_scale(C_, heads, self.c_ratio)

        def f32(t):
            return t.to(torch.float32).contiguous()

        def rows(w, b, hd):
            wn = torch.zeros((heads, HEAD_PAD) + tuple(w.shape[1:]), dtype=torch.float32, device=device)
            bn = torch.zeros((heads, HEAD_PAD), dtype=torch.float32, device=device)
            wn[:, :hd] = f32(w).reshape((heads, hd) + tuple(w.shape[1:]))
            if b is not None:
                bn[:, :hd] = f32(b).reshape(heads, hd)
            return wn.reshape((heads * HEAD_PAD,) + tuple(w.shape[1:])), bn.reshape(-1)

        wq, bq = rows(sd[f'{a}.q.weight'], sd.get(f'{a}.q.bias'), dq)
        wk, bk = rows(sd[f'{a}.k.weight'], sd.get(f'{a}.k.bias'), dq)
        wv, bv = rows(sd[f'{a}.v.weight'], sd.get(f'{a}.v.bias'), dv)
        cw = f32(sd[f'{a}.cpe.weight']).reshape(C_, 9).clone()
        cw[:, 4] += 1.0
        return {f'{a}.q': (wq * scale, bq * scale), f'{a}.kv': (torch.cat([wk, wv]), torch.cat([bk, bv])),
                f'{a}.cpe': (pad_heads(cw, heads), pad_heads(f32(sd[f'{a}.cpe.bias']), heads))}  # fmt: skip

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per input pixel at the 512 x 512 key count (1,024 pooled tokens); depthwise and pooled-map work included."""
        C_, hid, cr = self.embed_dim, self.hidden, self.cr
        ntok = self.split_size[0] * self.split_size[1]
        macs = 9 * self.in_chans * C_
        resi = tail_macs(C_, self.resi)
        for d in self.depth:
            for j in range(d):
                if j % 2 == 0:
                    macs += 3 * C_ * C_ + C_ * C_ + 9 * C_ + 2 * ntok * C_ // 2
                else:
                    heads = 1  # per-head widths sum to cr (q . k) and C (p . v)
                    macs += C_ * cr + C_ * C_ + 1024 * heads * (cr + C_) + C_ // 16 + (9 * C_ + C_ * cr + cr * cr + cr * C_ + 9 * C_) // 256
                macs += C_ * hid + 9 * (hid // 2) + (hid // 2) * C_
            macs += resi
        return macs + resi + pixelshuffle_macs(C_, 64, self.in_chans, self.upscale)

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, H, Wd = x_shape
        if c != self.in_chans:
            raise RuntimeError(f'model expects {self.in_chans} input channels, got {c}')
        C_, s, cr = self.embed_dim, self.upscale, self.cr
        has_rg = any(d >= 2 for d in self.depth)
        if has_rg:  # where the reference raises, before any launch
            t = rg_times(H, Wd)
            hs, ws = H // 4**t, Wd // 4**t
            if hs < 1 or ws < 1:
                raise RuntimeError(f'RG-SA: a {H}x{Wd} input reduces to {hs}x{ws} after {t} recursions of the 4x4 stride-4 convolution')
        with_lo = products == 3
        prod, fmt = int(products), products.fmt
        cp = (C_ + 7) // 8
        crp = (cr + 7) // 8
        half = self.hidden // 2
        P1 = (half + 7) // 8
        dev = plan.device
        max_heads = max(self.num_heads)
        hp_max = max_heads * HEAD_PAD // 8

        x_pl = plan.planes(n, (c + 7) // 8, H, Wd, with_lo)
        mean = W['mean']

        def set_input(x):
            ops.nchw_to_planes(x, x_pl, mean, self.img_range)  # (x - mean) * img_range (arch.py:828-829)

        first = plan.f32map(n, C_, H, Wd)
        pool = [plan.f32map(n, C_, H, Wd) for _ in range(4)]
        a_pl = plan.planes(n, cp, H, Wd, with_lo)
        qkv_pl = plan.planes(n, 3 * hp_max, H, Wd, with_lo)
        cat_pl = plan.planes(n, 2 * hp_max, H, Wd, with_lo)  # attention output | depthwise conv of v
        hid_pl = plan.planes(n, 2 * P1, H, Wd, with_lo)
        gate_pl = plan.planes(n, P1, H, Wd, with_lo)
        body_pl = plan.planes(n, cp, H, Wd, with_lo)
        resi_conv = ResidualTail(plan, W, self.resi, n, H, Wd, C_, with_lo)
        stats = torch.empty((n, H * Wd, 2), dtype=torch.float32, device=dev)
        plan.keep.append(stats)
        if has_rg:
            red_pl = plan.planes(n, cp, hs, ws, with_lo)
            dws_pl = plan.planes(n, cp, hs, ws, with_lo)
            cv_f32 = plan.f32map(n, cr, hs, ws)
            nrm_pl = plan.planes(n, crp, hs, ws, with_lo)
            kv_pl = plan.planes(n, 2 * hp_max, hs, ws, with_lo)
            v_pl = plan.planes(n, hp_max, hs, ws, with_lo)

        norm = layernorm_on(plan, W, n, H, Wd, C_)

        def rg_attention(a, heads):
            hp = heads * 4
            rp = L.RgReduceParams()  # reduction1 x t on the norm1 output
            rp.batch, rp.H, rp.W, rp.planes, rp.times, rp.fmt = n, H, Wd, cp, t, fmt
            a_pl.bind(rp, 'in')
            rp.weight, rp.bias = W[f'{a}.reduction1'][0].data_ptr(), W[f'{a}.reduction1'][1].data_ptr()
            red_pl.bind(rp, 'out')
            plan.launch('rsa_rg_reduce', rp)
            dwconv3x3(plan, W[f'{a}.dwconv'], red_pl, 0, cp, dws_pl)
            plan.conv(ops.conv_params(W[f'{a}.conv'], dws_pl, hs, ws, cin_planes=cp, out_f32=cv_f32))
            g, be = W[f'{a}.norm_act.0']
            lp = L.LayerNormParams()
            lp.batch, lp.H, lp.W, lp.C, lp.eps = n, hs, ws, cr, 1e-5
            lp.x_f32, lp.gamma, lp.beta = cv_f32.data_ptr(), g.data_ptr(), be.data_ptr()
            nrm_pl.bind(lp, 'out')
            lp.out_fmt = fmt
            plan.launch('rsa_layernorm_gelu', lp)
            plan.conv(ops.conv_params(W[f'{a}.kv'], nrm_pl, hs, ws, cin_planes=crp, out=kv_pl))
            dwconv3x3(plan, W[f'{a}.cpe'], kv_pl, hp, hp, v_pl)  # v + cpe(v)
            plan.conv(ops.conv_params(W[f'{a}.q'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
            ap = L.RgAttnParams()
            ap.batch, ap.H, ap.W, ap.heads, ap.nkeys = n, H, Wd, heads, hs * ws
            ap.dim_qk, ap.dim_v, ap.products, ap.fmt = cr // heads, C_ // heads, prod, fmt
            qkv_pl.bind(ap, 'q')
            kv_pl.bind(ap, 'k')
            v_pl.bind(ap, 'v')
            cat_pl.bind(ap, 'out')
            plan.launch('rsa_rg_attention', ap)

        def scale_add(res, gamma, out):
            plan.launch('rsa_scale_add', dict(res=res, gamma=gamma, out=out, batch=n, H=H, W=Wd, C=C_))

        plan.conv(ops.conv_params(W['conv_first'], x_pl, H, Wd, out_f32=first))
        free = list(pool)
        cur = free.pop()
        norm('before_RG.1', first, out_f32=cur)
        for i, d in enumerate(self.depth):
            heads = self.num_heads[i]
            hp = heads * 4
            rg_in = cur
            for j in range(d):
                b = f'layers.{i}.blocks.{j}'
                a = f'{b}.attn'
                norm(f'{b}.norm1', cur, out_planes=a_pl)
                x1 = free.pop()
                if j % 2 == 0:
                    plan.conv(ops.conv_params(W[f'{a}.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                    rect_attention(plan, qkv_pl, cat_pl, [W[f'{a}.bias{idx}'] for idx in (0, 1)], n, H, Wd, self.split_size, heads, is_shifted(i, j), prod, fmt)
                    dwconv3x3(plan, W[f'{a}.get_v'], qkv_pl, 2 * hp, hp, cat_pl, hp)
                    plan.conv(ops.conv_params(W[f'{a}.proj'], cat_pl, H, Wd, cin_planes=2 * hp, res1=cur, alpha=1.0, out_f32=x1))
                else:
                    rg_attention(a, heads)
                    plan.conv(ops.conv_params(W[f'{a}.proj'], cat_pl, H, Wd, cin_planes=hp, res1=cur, alpha=1.0, out_f32=x1))
                norm(f'{b}.norm2', x1, out_planes=a_pl)
                scale_add(cur, W[f'{b}.gamma'], x1)  # HAI: x1 + mlp(norm2(x1)) + gamma * res, once norm2 has read x1
                plan.conv(ops.conv_params(W[f'{b}.mlp.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
                sgw, sgb, sgg, sgbeta = W[f'{b}.mlp.sg']
                plane_stats(plan, hid_pl, P1, half, stats)
                dwconv3x3(plan, (sgw, sgb), hid_pl, P1, P1, gate_pl, stats=stats, gamma=sgg, beta=sgbeta, mul=hid_pl)
                x2 = free.pop()
                last = j == d - 1
                plan.conv(ops.conv_params(W[f'{b}.mlp.fc2'], gate_pl, H, Wd, cin_planes=P1, res1=x1, alpha=1.0, out_f32=x2,
                                          out=body_pl if last else None))  # fmt: skip
                if cur is not rg_in:
                    free.append(cur)
                free.append(x1)
                cur = x2
            out = free.pop()
            resi_conv(f'layers.{i}.conv', body_pl, rg_in, out_f32=out)
            free.append(rg_in)
            if cur is not rg_in:
                free.append(cur)
            cur = out
        norm('norm', cur, out_planes=a_pl)
        resi_conv('conv_after_body', a_pl, first, out_planes=body_pl)  # + conv_first output (arch.py:832)

        y_out = plan.output((n, self.in_chans, H * s, Wd * s), dtype)
        reconstruction_head(plan, W, 'pixelshuffle', body_pl, cp, n, H, Wd, s, with_lo, y_out, 1.0 / self.img_range, mean, None)  # x / img_range + mean
        return set_input
