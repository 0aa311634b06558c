"""HAT (Hybrid Attention Transformer) on the MI355X engine -- drop-in for ``resselt/archs/hat/arch.py:798-1110`` in eval mode.

Tokens are pixels, the residual stream is an f32 map, Linear layers are k1 launches of the convolution kernels:

  HAB  (arch.py:218-348)  LN -> { CAB: conv3x3 + GELU, conv3x3, channel attention (global mean -> 1x1 -> ReLU -> 1x1 -> sigmoid) }
                          and { qkv -> (shifted) 16x16 window attention -> proj };  x = shortcut + attn + CAB * 0.01;  LN -> MLP
  OCAB (arch.py:351-482)  LN -> qkv -> attention of every 16x16 window's queries over the 24x24 window around it (nn.Unfold with zero
                          padding) -> proj (+ shortcut);  LN -> MLP
  RHAG (arch.py:590-692)  blocks, one OCAB, conv3x3 (+ residual)

Both attention kinds run on ``rsa_rect_attention`` (csrc/dat.hip): the self-attention with its 256-token window resident in LDS, the
overlapping one in its cross-window mode (576 keys streamed through LDS in chunks of 256, flash-style state in registers).  The
relative-position tables are gathered once, at pack time, into the kernel's accumulator-fragment order.
"""

from __future__ import annotations

import os

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, PF_F16
from ...engine.transformer import (HEAD_PAD, LayerPacker, attn_tiles, bias_fragments_qk, layernorm_on, mlp_block, mlp_block_fits, pack_head,
                                   pixelshuffle_macs, reconstruction_head, regroup_proj, regroup_qkv, relative_position_index)

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # arch.py:842


def rpi_buffers(window: int, overlap_ratio: float):
    """``relative_position_index_SA`` / ``_OCA`` (arch.py:987-1034)."""
    co = torch.stack(torch.meshgrid([torch.arange(window), torch.arange(window)], indexing='ij')).flatten(1)
    ext = window + int(overlap_ratio * window)
    ce = torch.stack(torch.meshgrid([torch.arange(ext), torch.arange(ext)], indexing='ij')).flatten(1)
    rel = (ce[:, None, :] - co[:, :, None]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - ext + 1
    rel[:, :, 1] += window - ext + 1
    rel[:, :, 0] *= window + ext - 1
    return relative_position_index(window), rel.sum(-1)


def hat_param_shapes(in_chans, embed_dim, depths, num_heads, window, compress_ratio, squeeze_factor, overlap_ratio, mlp_ratio, upscale, num_feat,
                     resi, patch_norm, qkv_bias):  # fmt: skip
    s = ParamShapes()
    C_ = embed_dim
    hidden = int(C_ * mlp_ratio)
    ext = window + int(overlap_ratio * window)

    s.conv('conv_first', C_, in_chans, 3)
    if patch_norm:
        s.norm('patch_embed.norm', C_)
    for i, depth in enumerate(depths):
        g = f'layers.{i}.residual_group'
        for j in range(depth):
            b = f'{g}.blocks.{j}'
            s.norm(f'{b}.norm1', C_)
            s[f'{b}.attn.relative_position_bias_table'] = ((2 * window - 1) ** 2, num_heads[i])
            s.linear(f'{b}.attn.qkv', 3 * C_, C_, qkv_bias)
            s.linear(f'{b}.attn.proj', C_, C_)
            s.conv(f'{b}.conv_block.cab.0', int(C_ // compress_ratio), C_, 3)
            s.conv(f'{b}.conv_block.cab.2', C_, int(C_ // compress_ratio), 3)
            s.conv(f'{b}.conv_block.cab.3.attention.1', int(C_ // squeeze_factor), C_, 1)
            s.conv(f'{b}.conv_block.cab.3.attention.3', C_, int(C_ // squeeze_factor), 1)
            s.norm(f'{b}.norm2', C_)
            s.linear(f'{b}.mlp.fc1', hidden, C_)
            s.linear(f'{b}.mlp.fc2', C_, hidden)
        o = f'{g}.overlap_attn'
        s.norm(f'{o}.norm1', C_)
        s.linear(f'{o}.qkv', 3 * C_, C_, qkv_bias)
        s[f'{o}.relative_position_bias_table'] = ((window + ext - 1) ** 2, num_heads[i])
        s.linear(f'{o}.proj', C_, C_)
        s.norm(f'{o}.norm2', C_)
        s.linear(f'{o}.mlp.fc1', hidden, C_)
        s.linear(f'{o}.mlp.fc2', C_, hidden)
        if resi == '1conv':
            s.conv(f'layers.{i}.conv', C_, C_, 3)
    s.norm('norm', C_)
    if resi == '1conv':
        s.conv('conv_after_body', C_, C_, 3)
    s.pixelshuffle_head(C_, num_feat, in_chans, upscale)
    sa, oca = rpi_buffers(window, overlap_ratio)
    return s, {'relative_position_index_SA': sa, 'relative_position_index_OCA': oca}


class HAT(EngineModule):
    hyperparameters = {}
    # 'mixed' (what 'auto' selects when the MLP halves run the fused kernel): everything between two reads of the f32 token stream -- qkv, the
    # window / overlapping cross-window attention, proj, the CAB's two 3x3 convolutions and the fused norm2 + fc1 + GELU + fc2 half -- runs ONE
    # fp16 product on hi planes; the group / head convolutions keep three bf16 products.
    precisions = ('bf16x3', 'bf16', 'mixed')
    precision_table = {'mixed': (3, PF_BF16)}

    @property
    def auto_precision(self) -> str:
        return 'mixed'

    @staticmethod
    def layer_policy(name: str) -> tuple[int, int]:
        """(products, plane format of inputs and weights) of layer ``name`` under 'mixed'."""
        if name.endswith(('.qkv', '.proj', '.mlp.fc1', '.mlp.fc2')) or '.conv_block.cab.' in name:
            return 1, PF_F16
        return 3, PF_BF16

    fused_mlp = os.environ.get('RSA_HAT_FUSED_MLP', '1') != '0'  # LayerNorm + fc1 + GELU + fc2 + shortcut as one launch where the widths allow it (engine/transformer.py)

    def __init__(self, *, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, ape=False, patch_norm=True, use_checkpoint=False, upscale=1,
                 img_range=1.0, upsampler='pixelshuffle', resi_connection='1conv', num_feat=64) -> None:  # fmt: skip
        super().__init__()
        if patch_size != 1 or ape or qk_scale is not None or upsampler != 'pixelshuffle':
            raise NotImplementedError('HAT engine supports patch_size=1, ape=False, default qk scale, pixelshuffle (what the loader builds)')
        depths, num_heads = list(depths), list(num_heads)
        ext = window_size + int(overlap_ratio * window_size)
        if window_size * window_size > 256 or (ext - window_size) % 2:
            raise NotImplementedError('window_size must be <= 16 and the overlap symmetric')
        if any(embed_dim % h or embed_dim // h > HEAD_PAD for h in num_heads) or embed_dim % 4 or num_feat % 8:
            raise NotImplementedError('head_dim must divide embed_dim and be <= 32; embed_dim % 4 == 0; num_feat % 8 == 0')
        if int(embed_dim // squeeze_factor) < 1 or int(embed_dim // squeeze_factor) > 64:
            raise NotImplementedError('channel-attention width must be in 1..64')
        self.in_chans, self.embed_dim, self.depths, self.num_heads = in_chans, embed_dim, depths, num_heads
        self.window_size, self.ext, self.mlp_ratio, self.conv_scale = window_size, ext, mlp_ratio, conv_scale
        self.compress, self.upscale, self.img_range, self.resi = int(embed_dim // compress_ratio), upscale, img_range, resi_connection
        self.patch_norm, self.num_feat, self.img_size = patch_norm, num_feat, img_size
        shapes, buffers = hat_param_shapes(in_chans, embed_dim, depths, num_heads, window_size, compress_ratio, squeeze_factor, overlap_ratio,
                                           mlp_ratio, upscale, num_feat, resi_connection, patch_norm, qkv_bias)  # fmt: skip
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device) for k, v in self.state_dict().items()}
        C_, ws, ext = self.embed_dim, self.window_size, self.ext
        cp = (C_ + 7) // 8
        pk = LayerPacker(sd, device, products, self.layer_policy)
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln

        def f32(t):
            return t.to(torch.float32).contiguous()

        def attention(name, heads, table_key, rpi, nq, nk, cross):
            wq, bq = regroup_qkv(sd[f'{name}.qkv.weight'], sd.get(f'{name}.qkv.bias'), heads)
            lin(f'{name}.qkv', wq, bq)
            lin(f'{name}.proj', regroup_proj(sd[f'{name}.proj.weight'], heads), sd[f'{name}.proj.bias'], cin_planes=heads * HEAD_PAD // 8)
            dense = f32(sd[table_key])[rpi.reshape(-1).long()].view(nq, nk, heads).permute(2, 0, 1)
            qt = (nq + 31) // 32 if cross else attn_tiles(nq)
            kt = (nk + 31) // 32 if cross else attn_tiles(nk)
            W[f'{name}.bias_frag'] = bias_fragments_qk(dense, qt, kt)

        def pad_cols(t, n):
            out = torch.zeros((t.shape[0], n), dtype=torch.float32, device=device)
            out[:, : t.shape[1]] = t
            return out.contiguous()

        def pad_rows(t, n):
            out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=torch.float32, device=device)
            out[: t.shape[0]] = t
            return out.contiguous()

        conv('conv_first')
        if self.patch_norm:
            ln('patch_embed.norm')
        rpi_sa, rpi_oca = sd['relative_position_index_SA'], sd['relative_position_index_OCA']
        for i, depth in enumerate(self.depths):
            heads = self.num_heads[i]
            g = f'layers.{i}.residual_group'
            for j in range(depth):
                b = f'{g}.blocks.{j}'
                ln(f'{b}.norm1')
                ln(f'{b}.norm2')
                attention(f'{b}.attn', heads, f'{b}.attn.relative_position_bias_table', rpi_sa, ws * ws, ws * ws, False)
                conv(f'{b}.conv_block.cab.0')
                conv(f'{b}.conv_block.cab.2')
                w1 = f32(sd[f'{b}.conv_block.cab.3.attention.1.weight']).reshape(-1, C_)
                w2 = f32(sd[f'{b}.conv_block.cab.3.attention.3.weight']).reshape(C_, -1)
                W[f'{b}.ca'] = (pad_cols(w1, cp * 8), f32(sd[f'{b}.conv_block.cab.3.attention.1.bias']), pad_rows(w2, cp * 8),
                                pad_rows(f32(sd[f'{b}.conv_block.cab.3.attention.3.bias']), cp * 8))  # fmt: skip
                lin(f'{b}.mlp.fc1')
                lin(f'{b}.mlp.fc2')
            o = f'{g}.overlap_attn'
            ln(f'{o}.norm1')
            ln(f'{o}.norm2')
            attention(o, heads, f'{o}.relative_position_bias_table', rpi_oca, ws * ws, ext * ext, True)
            lin(f'{o}.mlp.fc1')
            lin(f'{o}.mlp.fc2')
            if self.resi == '1conv':
                conv(f'layers.{i}.conv')
        ln('norm')
        if self.resi == '1conv':
            conv('conv_after_body')
        else:  # 'identity': the residual adds still run as (exact) identity k1 launches
            W['identity'] = ops.ConvWeights.from_oihw(torch.eye(C_, device=device)[:, :, None, None], None, int(products), device=device, fmt=products.fmt)
        pack_head(pk)
        check_fp16_range(W.values())
        W['mean'] = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=device)
        return W

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per (window-padded) input pixel."""
        C_, ws, ext = self.embed_dim, self.window_size, self.ext
        hidden = int(C_ * self.mlp_ratio)
        macs = 9 * self.in_chans * C_
        for depth in self.depths:
            macs += depth * (4 * C_ * C_ + 2 * ws * ws * C_ + 2 * 9 * C_ * self.compress + 2 * C_ * hidden)
            macs += 4 * C_ * C_ + 2 * ext * ext * C_ + 2 * C_ * hidden
            macs += 9 * C_ * C_ if self.resi == '1conv' else 0
        macs += 9 * C_ * C_ if self.resi == '1conv' else 0
        return macs + pixelshuffle_macs(C_, self.num_feat, self.in_chans, self.upscale)

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, h0, w0 = x_shape
        if c != self.in_chans:
            raise RuntimeError(f'model expects {self.in_chans} input channels, got {c}')
        ws, ext = self.window_size, self.ext
        H, Wd = h0 + (ws - h0 % ws) % ws, w0 + (ws - w0 % ws) % ws
        if H - h0 >= h0 or Wd - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to a multiple of the window size')
        C_, s, nf = self.embed_dim, self.upscale, self.num_feat
        hidden = int(C_ * self.mlp_ratio)
        with_lo = products == 3
        cp = (C_ + 7) // 8
        dev = plan.device
        lib = L.load()
        max_heads = max(self.num_heads)

        x_pl = plan.planes(n, (c + 7) // 8, H, Wd, with_lo)
        mean = W['mean']

        def set_input(x):
            ops.nchw_to_planes(x, x_pl, mean, self.img_range)  # (x - mean) * img_range and check_image_size's reflect padding (arch.py:1091-1101)

        first = plan.f32map(n, C_, H, Wd)
        pool = [plan.f32map(n, C_, H, Wd) for _ in range(5)]
        mixed = products.name == 'mixed'
        one = dict(with_lo=False, fmt=PF_F16) if mixed else dict(with_lo=with_lo)  # what a one-product layer reads: an fp16 hi plane
        a_pl = plan.planes(n, cp, H, Wd, **one)  # norm1 -> qkv and the CAB
        n_pl = plan.planes(n, cp, H, Wd, with_lo) if mixed else a_pl  # the last LayerNorm -> conv_after_body (three products)
        qkv_pl = plan.planes(n, 3 * max_heads * HEAD_PAD // 8, H, Wd, **one)
        o_pl = plan.planes(n, max_heads * HEAD_PAD // 8, H, Wd, **one)
        fuse_mlp = self.fused_mlp and mlp_block_fits(C_, hidden)
        hid_pl = None if fuse_mlp else plan.planes(n, (hidden + 7) // 8, H, Wd, **one)
        body_pl = plan.planes(n, cp, H, Wd, with_lo)
        cab_a = plan.planes(n, (self.compress + 7) // 8, H, Wd, **one)
        cab_b = plan.planes(n, cp, H, Wd, with_lo)
        gate = torch.empty((n, cp * 8), dtype=torch.float32, device=dev)
        ws_gate = torch.empty((max(int(lib.rsa_channel_gate_workspace_bytes(n, H, Wd, cp)), 16) // 4,), dtype=torch.float32, device=dev)
        plan.keep += [gate, ws_gate]

        norm = layernorm_on(plan, W, n, H, Wd, C_)

        def attention(name, heads, shift, cross):
            ap = L.RectAttnParams()
            ap.batch, ap.H, ap.W, ap.Hp, ap.Wp = n, H, Wd, H, Wd
            ap.win_h, ap.win_w, ap.shift_h, ap.shift_w = ws, ws, shift, shift
            ap.heads, ap.head0, ap.heads_total, ap.products = heads, 0, heads, (1 if mixed else int(products))
            ap.fmt = qkv_pl.fmt
            qkv_pl.bind(ap, 'qkv')
            ap.bias_frag = W[f'{name}.bias_frag'].data_ptr()
            o_pl.bind(ap, 'out')
            if cross:
                ap.kwin_h = ap.kwin_w = ext
                ap.kpad_h = ap.kpad_w = (ext - ws) // 2
            plan.launch('rsa_rect_attention', ap)

        def cab_scaled_shortcut(b, shortcut, out_f32):
            """out = shortcut + CAB(LN(x)) * conv_scale, CAB = conv-GELU-conv followed by its channel attention (arch.py:37-59, 345)."""
            plan.conv(ops.conv_params(W[f'{b}.conv_block.cab.0'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=cab_a))
            plan.conv(ops.conv_params(W[f'{b}.conv_block.cab.2'], cab_a, H, Wd, out=cab_b))
            w1, b1, w2, b2 = W[f'{b}.ca']
            gp = L.ChannelGateParams()
            gp.batch, gp.H, gp.W, gp.planes, gp.hidden, gp.relu = n, H, Wd, cp, w1.shape[0], 1
            cab_b.bind(gp, 'in')
            gp.w1, gp.b1, gp.w2, gp.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
            gp.workspace, gp.gate = ws_gate.data_ptr(), gate.data_ptr()
            plan.launch('rsa_channel_gate', gp, kernels=2)
            plan.launch('rsa_gated_add', dict(x_hi=cab_b.hi_ptr(), x_lo=cab_b.lo_ptr(), plane_stride=cab_b.plane_stride, batch_stride=cab_b.batch_stride,
                                              batch=n, H=H, W=Wd, C=C_, gate=gate, scale=self.conv_scale, base_f32=shortcut, out_f32=out_f32))  # fmt: skip

        def mlp(b, x1, x2, out_planes=None):
            if fuse_mlp:  # one launch (csrc/swin_block.hip), nothing between leaves the chip
                mlp_block(plan, W[f'{b}.norm2'], W[f'{b}.mlp.fc1'], W[f'{b}.mlp.fc2'], n, H, Wd, C_, hidden, products, x1, x2, out_planes)
                return
            norm(f'{b}.norm2', x1, out_planes=a_pl)
            plan.conv(ops.conv_params(W[f'{b}.mlp.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
            plan.conv(ops.conv_params(W[f'{b}.mlp.fc2'], hid_pl, H, Wd, cin_planes=(hidden + 7) // 8, res1=x1, alpha=1.0, out_f32=x2, out=out_planes))

        plan.conv(ops.conv_params(W['conv_first'], x_pl, H, Wd, out_f32=first))
        free = list(pool)
        if self.patch_norm:
            cur = free.pop()
            norm('patch_embed.norm', first, out_f32=cur)
        else:
            cur = first
        for i, depth in enumerate(self.depths):
            heads = self.num_heads[i]
            hp = heads * HEAD_PAD // 8
            g = f'layers.{i}.residual_group'
            rg_in = cur

            def release(t):
                if t is not rg_in and t is not first:
                    free.append(t)

            for j in range(depth):
                b = f'{g}.blocks.{j}'
                norm(f'{b}.norm1', cur, out_planes=a_pl)
                sc = free.pop()
                cab_scaled_shortcut(b, cur, sc)
                plan.conv(ops.conv_params(W[f'{b}.attn.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                attention(f'{b}.attn', heads, 0 if j % 2 == 0 else ws // 2, False)
                x1 = free.pop()
                plan.conv(ops.conv_params(W[f'{b}.attn.proj'], o_pl, H, Wd, cin_planes=hp, res1=sc, alpha=1.0, out_f32=x1))
                free.append(sc)
                x2 = free.pop()
                mlp(b, x1, x2)
                release(cur)
                free.append(x1)
                cur = x2
            o = f'{g}.overlap_attn'
            norm(f'{o}.norm1', cur, out_planes=a_pl)
            plan.conv(ops.conv_params(W[f'{o}.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
            attention(o, heads, 0, True)
            x1 = free.pop()
            plan.conv(ops.conv_params(W[f'{o}.proj'], o_pl, H, Wd, cin_planes=hp, res1=cur, alpha=1.0, out_f32=x1))
            x2 = free.pop()
            mlp(o, x1, x2, out_planes=body_pl)
            release(cur)
            free.append(x1)
            cur = x2
            out = free.pop()
            tail = W[f'layers.{i}.conv'] if self.resi == '1conv' else W['identity']
            plan.conv(ops.conv_params(tail, body_pl, H, Wd, cin_planes=cp, res1=rg_in, alpha=1.0, out_f32=out))
            if rg_in is not first:
                free.append(rg_in)
            free.append(cur)
            cur = out
        norm('norm', cur, out_planes=n_pl)
        tail = W['conv_after_body'] if self.resi == '1conv' else W['identity']
        plan.conv(ops.conv_params(tail, n_pl, H, Wd, cin_planes=cp, res1=first, alpha=1.0, out=body_pl))  # + conv_first output (arch.py:1104)

        y_out = plan.output((n, self.in_chans, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        reconstruction_head(plan, W, 'pixelshuffle', body_pl, cp, n, H, Wd, s, with_lo, y_out, 1.0 / self.img_range, mean, None, nf=nf)
        return set_input
