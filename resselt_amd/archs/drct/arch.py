"""DRCT (Dense-residual-connected Transformer) on the MI355X engine -- drop-in for ``resselt/archs/drct/arch.py:617-792``.

Reference structure: conv_first -> [patch_embed.norm] -> RDG x num_layers -> norm -> conv_after_body (+ conv_first) ->
conv_before_upsample -> Upsample (conv + PixelShuffle) -> conv_last.  A dense group (RDG, arch.py:204-329) is five Swin blocks over a
growing channel concatenation -- widths dim, dim+gc, ..., dim+4gc, with ``num_heads - width % num_heads`` heads, i.e. head widths of
30..122 channels for the published dim 180 / gc 32 / 6 heads -- each followed by a 1x1 'adjust' convolution, and ``x5 * 0.2 + x``.

On the engine:
  * the concatenation ``torch.cat((x, x1, ..), -1)`` is ONE f32 token map of dim + 4gc channels: channel groups of 4 are the unit of
    that layout, dim and gc are multiples of 4, so every adjust convolution stores its gc channels at a group offset and a block of
    width w reads the first w channels (LayerNorm, residual) -- no copy.  (That addressing holds for one image per call.)
  * a Swin block is LayerNorm -> qkv (k1) -> rsa_rect_attention with 16x16 windows and ``head_chunks`` = ceil(head_dim / 32) chunks of
    32 channels per head (csrc/dat.hip, wide-head kernel) -> proj (+ shortcut) -> LayerNorm -> fc1 (GELU) -> fc2 (+ shortcut), all Linear
    layers as k1 launches of the convolution kernels; the shift mask is index arithmetic on the actual (padded) size.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, PF_F16, Planes
from ...engine.transformer import (LayerPacker, bias_fragments_qk, layernorm, pack_head, pixelshuffle_buffers, pixelshuffle_head, pixelshuffle_macs,
                                   regroup_proj, regroup_qkv, relative_position_index, shift_mask)

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # arch.py:649

# names this module exported before the shared helpers moved to engine/transformer.py
regroup_qkv_wide, regroup_proj_wide = regroup_qkv, regroup_proj


def block_dims(embed_dim: int, gc: int, num_heads: int):
    """(width, heads, shifted, mlp uses mlp_ratio) of the five Swin blocks of a dense group (arch.py:225-298)."""
    out = []
    for j in range(5):
        dim = embed_dim + j * gc
        heads = num_heads if j == 0 else num_heads - (dim % num_heads)
        out.append((dim, heads, j in (1, 3), j < 3))
    return out


def drct_param_shapes(in_chans, embed_dim, num_layers, num_heads, window, mlp_ratio, gc, upscale, resi, img_size, patch_norm, qkv_bias, upsampler):
    s = ParamShapes()
    buffers: dict = {}
    C_ = embed_dim

    s.conv('conv_first', C_, in_chans, 3)
    if patch_norm:
        s.norm('patch_embed.norm', C_)
    for i in range(num_layers):
        for j, (dim, heads, shifted, full_mlp) in enumerate(block_dims(C_, gc, num_heads[i]), start=1):
            b = f'layers.{i}.swin{j}'
            hidden = int(dim * (mlp_ratio if full_mlp else 1))
            s.norm(f'{b}.norm1', dim)
            s[f'{b}.attn.relative_position_bias_table'] = ((2 * window - 1) ** 2, heads)
            buffers[f'{b}.attn.relative_position_index'] = relative_position_index(window)
            if shifted and img_size > window:
                buffers[f'{b}.attn_mask'] = shift_mask(img_size, img_size, (window, window), (window // 2, window // 2))
            s.linear(f'{b}.attn.qkv', 3 * dim, dim, qkv_bias)
            s.linear(f'{b}.attn.proj', dim, dim)
            s.norm(f'{b}.norm2', dim)
            s.linear(f'{b}.mlp.fc1', hidden, dim)
            s.linear(f'{b}.mlp.fc2', dim, hidden)
            s.conv(f'layers.{i}.adjust{j}', gc if j < 5 else C_, dim, 1)
    s.norm('norm', C_)
    if resi == '1conv':
        s.conv('conv_after_body', C_, C_, 3)
    if upsampler == 'pixelshuffle':
        s.pixelshuffle_head(C_, 64, in_chans, upscale)
    return s, buffers


class DRCT(EngineModule):
    hyperparameters = {}
    # 'mixed' (what 'auto' selects): every Linear layer of a dense group (qkv, proj, fc1, fc2, the 1x1 `adjust` convolutions) and the window
    # attention between them -- all of it feeding the f32 token stream through the next LayerNorm -- run ONE fp16 product on hi planes
    # (LayerNorm outputs, q / k / v, softmax probabilities, attention outputs, hidden activations and block outputs are fp16 hi planes: 2
    # bytes per channel instead of 4).  The 3x3 convolutions (conv_first, conv_after_body, the reconstruction head) run three bf16 products
    # as in RRDBNet's tail.
    auto_precision = 'mixed'
    precisions = ('bf16x3', 'bf16', 'mixed')
    precision_table = {'mixed': (3, PF_BF16)}

    @staticmethod
    def layer_policy(name: str) -> tuple[int, int]:
        """(products, plane format of inputs and weights) of layer ``name`` under 'mixed'."""
        if name.endswith(('.attn.qkv', '.attn.proj', '.mlp.fc1', '.mlp.fc2')) or '.adjust' in name:
            return 1, PF_F16
        return 3, PF_BF16

    def __init__(self, *, img_size=64, patch_size=1, in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6),
                 window_size=16, mlp_ratio=2.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1,
                 ape=False, patch_norm=True, upscale=1, img_range=1.0, upsampler='', resi_connection='1conv', gc=32) -> None:  # fmt: skip
        super().__init__()
        if patch_size != 1 or ape or qk_scale is not None:
            raise NotImplementedError('DRCT engine supports patch_size=1, ape=False, default qk scale (what the loader builds)')
        if upsampler != 'pixelshuffle':
            raise NotImplementedError("DRCT reconstructs only with upsampler='pixelshuffle' (the reference forward returns its input otherwise)")
        if embed_dim % 4 or gc % 4:
            raise NotImplementedError('embed_dim and gc must be multiples of 4 (channel groups of the f32 token map)')
        if window_size * window_size > 256:
            raise NotImplementedError('window must hold at most 256 tokens')
        if img_size < window_size:
            raise NotImplementedError('img_size < window_size shrinks the window (and its bias table) to the image size; not supported')
        # img_size == window_size is what the loader passes for a checkpoint saved without attn_mask buffers (drct/__init__.py:78-82 of the
        # reference): a block whose input_resolution <= window drops its shift (drct/arch.py:373-376), so swin2 / swin4 run unshifted
        self.unshifted = img_size == window_size
        if resi_connection not in ('1conv', 'identity'):
            raise NotImplementedError(f"resi_connection must be '1conv' or 'identity', got {resi_connection!r}")
        num_heads = list(num_heads)
        for nh in num_heads:
            for dim, heads, _, _ in block_dims(embed_dim, gc, nh):
                if heads < 1 or dim % heads or dim // heads > 128:
                    raise NotImplementedError(f'block width {dim} with {heads} heads: head_dim must divide the width and be <= 128')
        self.in_chans, self.embed_dim, self.num_heads, self.num_layers = in_chans, embed_dim, num_heads, len(num_heads)
        self.window_size, self.mlp_ratio, self.gc = window_size, mlp_ratio, gc
        self.upscale, self.img_range, self.resi, self.patch_norm, self.qkv_bias = upscale, img_range, resi_connection, patch_norm, qkv_bias
        shapes, buffers = drct_param_shapes(in_chans, embed_dim, self.num_layers, num_heads, window_size, mlp_ratio, gc, upscale, resi_connection,
                                            img_size, patch_norm, qkv_bias, upsampler)  # fmt: skip
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device) for k, v in self.state_dict().items()}
        pk = LayerPacker(sd, device, products, self.layer_policy)
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln

        conv('conv_first')
        if self.patch_norm:
            ln('patch_embed.norm')
        win = self.window_size
        for i in range(self.num_layers):
            for j, (dim, heads, _, _) in enumerate(block_dims(self.embed_dim, self.gc, self.num_heads[i]), start=1):
                b = f'layers.{i}.swin{j}'
                pad = 32 * -(-(dim // heads) // 32)
                ln(f'{b}.norm1')
                ln(f'{b}.norm2')
                wq, bq = regroup_qkv(sd[f'{b}.attn.qkv.weight'], sd.get(f'{b}.attn.qkv.bias'), heads, pad)
                lin(f'{b}.attn.qkv', wq, bq)
                lin(f'{b}.attn.proj', regroup_proj(sd[f'{b}.attn.proj.weight'], heads, pad), sd[f'{b}.attn.proj.bias'], cin_planes=heads * pad // 8)
                lin(f'{b}.mlp.fc1')
                lin(f'{b}.mlp.fc2')
                n = win * win
                dense = sd[f'{b}.attn.relative_position_bias_table'].float()[sd[f'{b}.attn.relative_position_index'].reshape(-1).long()]
                W[f'{b}.bias_frag'] = bias_fragments_qk(dense.reshape(n, n, heads).permute(2, 0, 1).contiguous())
                conv(f'layers.{i}.adjust{j}')
        ln('norm')
        if self.resi == 'identity':  # nn.Identity as a 1x1 convolution (see _build_plan)
            eye = torch.eye(self.embed_dim, dtype=torch.float32, device=device)[:, :, None, None]
            W['identity'] = ops.ConvWeights.from_oihw(eye, torch.zeros(self.embed_dim, dtype=torch.float32, device=device), int(products), device=device, fmt=products.fmt)
        if self.resi == '1conv':
            conv('conv_after_body')
        pack_head(pk)
        check_fp16_range(W.values())
        W['mean'] = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=device)
        return W

    def macs_per_input_pixel(self) -> int:
        """Algorithmic multiply-accumulates per pixel of the (window-padded) input grid: Linear layers, QK^T + PV over a window, the 1x1
        adjust convolutions, and the convolutions of the head at their own resolution."""
        C_, gc, n_tok = self.embed_dim, self.gc, self.window_size**2
        total = 9 * self.in_chans * C_
        for nh in self.num_heads:
            for j, (dim, heads, _, full_mlp) in enumerate(block_dims(C_, gc, nh), start=1):
                hidden = int(dim * (self.mlp_ratio if full_mlp else 1))
                total += 4 * dim * dim + 2 * n_tok * dim + 2 * dim * hidden + dim * (gc if j < 5 else C_)
        if self.resi == '1conv':
            total += 9 * C_ * C_
        return total + pixelshuffle_macs(C_, 64, self.in_chans, self.upscale)

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        """One plan per input signature.  The dense concatenation of a group is addressed by channel-group views inside ONE image's token
        map, so a batch is the per-image launch list repeated over the images of the batch, all sharing one set of intermediate buffers
        (the launches of a plan run in order on one stream); only the input planes and the output tensor are per image."""
        nb, c, h0, w0 = x_shape
        if c != self.in_chans:
            raise RuntimeError(f'model expects {self.in_chans} input channels, got {c}')
        n = 1  # images per launch
        win = self.window_size
        H, Wd = h0 + (win - h0 % win) % win, w0 + (win - w0 % win) % win
        if H - h0 >= h0 or Wd - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to a multiple of the window size')
        C_, gc, s = self.embed_dim, self.gc, self.upscale
        wide = C_ + 4 * gc
        with_lo = products == 3
        dev = plan.device

        x_all = plan.planes(nb, (c + 7) // 8, H, Wd, with_lo)
        mean = W['mean']

        def set_input(x):
            # (x - mean) * img_range and check_img_size's reflect padding (arch.py:765-776), fused into the layout kernel
            ops.nchw_to_planes(x, x_all, mean, self.img_range)

        first = plan.f32map(n, C_, H, Wd)
        cat = [plan.f32map(n, wide, H, Wd) for _ in range(2)]  # dense concatenation of a group: x | x1 | x2 | x3 | x4
        blk = [plan.f32map(n, wide, H, Wd) for _ in range(2)]  # a Swin block's two residual sums
        max_pad = max(heads * 32 * -(-(dim // heads) // 32) for nh in self.num_heads for dim, heads, _, _ in block_dims(C_, gc, nh))
        mixed = products.name == 'mixed'
        # 'mixed': what a one-product layer (Linear or attention) reads is an fp16 hi plane (2 bytes per channel); what the 3x3 convolutions
        # read stays bf16 hi + lo
        one = dict(with_lo=False, fmt=PF_F16) if mixed else dict(with_lo=with_lo)
        a_pl = plan.planes(n, (wide + 7) // 8, H, Wd, **one)  # LayerNorm outputs -> qkv / fc1
        n_pl = plan.planes(n, (C_ + 7) // 8, H, Wd, with_lo) if mixed else a_pl  # the last LayerNorm -> conv_after_body (three products)
        qkv_pl = plan.planes(n, 3 * max_pad // 8, H, Wd, **one)
        o_pl = plan.planes(n, max_pad // 8, H, Wd, **one)
        hid_pl = plan.planes(n, (int(wide * max(self.mlp_ratio, 1.0)) + 7) // 8, H, Wd, **one)
        t_pl = plan.planes(n, (wide + 7) // 8, H, Wd, **one)  # a block's output as planes (input of its adjust convolution)
        body_pl = plan.planes(n, (C_ + 7) // 8, H, Wd, with_lo)
        head = pixelshuffle_buffers(plan, W, n, H, Wd, 64, with_lo)  # shared by the images of a batch
        if self.resi == 'identity' and 'identity' not in W:
            raise RuntimeError('packed weights lack the identity layer')  # (_pack adds it)

        def chan_view(m: torch.Tensor, c0: int, cn: int) -> torch.Tensor:
            """Channels [c0, c0 + cn) of an f32 token map as a map of their own (one image: groups are contiguous)."""
            return m[:, c0 // 4 : (c0 + cn) // 4]

        def norm(name, x_f32, C_in, out_planes=None, out_f32=None):
            layernorm(plan, W, name, n, H, Wd, C_in, x_f32, out_planes, out_f32)

        def attention(name, heads, chunks, shifted):
            ap = L.RectAttnParams()
            ap.batch, ap.H, ap.W, ap.Hp, ap.Wp = n, H, Wd, H, Wd
            ap.win_h = ap.win_w = win
            ap.shift_h = ap.shift_w = win // 2 if shifted else 0
            ap.heads, ap.head0, ap.heads_total, ap.products, ap.head_chunks = heads, 0, heads, (1 if mixed else int(products)), chunks
            ap.fmt = qkv_pl.fmt
            qkv_pl.bind(ap, 'qkv')
            ap.bias_frag = W[f'{name}.bias_frag'].data_ptr()
            o_pl.bind(ap, 'out')
            plan.launch('rsa_rect_attention', ap)

        def f32_view_conv(wts, src, **kw):
            """conv_params with f32 operands that are channel views of wider maps: checked against the view, passed by pointer."""
            return ops.conv_params(wts, src, H, Wd, **kw)

        y_out = plan.output((nb, self.in_chans, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        final = dict(out_scale=1.0 / self.img_range, out_shift=mean)  # x / img_range + mean (arch.py:790)

        def image(bi: int) -> None:
            x_pl = Planes(x_all.hi[bi : bi + 1], None if x_all.lo is None else x_all.lo[bi : bi + 1])
            plan.conv(ops.conv_params(W['conv_first'], x_pl, H, Wd, out_f32=first))
            cur = cat[0]
            if self.patch_norm:
                norm('patch_embed.norm', first, C_, out_f32=chan_view(cur, 0, C_))
            else:
                plan.call(lambda dst=chan_view(cur, 0, C_): dst.copy_(first))
            ci = 0
            for i in range(self.num_layers):
                cur, nxt = cat[ci], cat[ci ^ 1]
                for j, (dim, heads, shifted, full_mlp) in enumerate(block_dims(C_, gc, self.num_heads[i]), start=1):
                    b = f'layers.{i}.swin{j}'
                    chunks = -(-(dim // heads) // 32)
                    hp = heads * 32 * chunks // 8
                    cp = (dim + 7) // 8
                    hidden = int(dim * (self.mlp_ratio if full_mlp else 1))
                    xin = chan_view(cur, 0, dim)
                    norm(f'{b}.norm1', xin, dim, out_planes=a_pl)
                    plan.conv(ops.conv_params(W[f'{b}.attn.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                    attention(b, heads, chunks, shifted and not self.unshifted)
                    x1 = chan_view(blk[0], 0, dim)
                    plan.conv(f32_view_conv(W[f'{b}.attn.proj'], o_pl, cin_planes=hp, res1=xin, alpha=1.0, out_f32=x1))
                    norm(f'{b}.norm2', x1, dim, out_planes=a_pl)
                    plan.conv(ops.conv_params(W[f'{b}.mlp.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
                    plan.conv(f32_view_conv(W[f'{b}.mlp.fc2'], hid_pl, cin_planes=(hidden + 7) // 8, res1=x1, alpha=1.0, out=t_pl))
                    # adjust_j (1x1) on the block's output: x_j = lrelu(.) stored at channel offset dim of the concatenation;
                    # adjust_5 closes the group: x5 * 0.2 + x into the first C_ channels of the next group's concatenation
                    if j < 5:
                        plan.conv(f32_view_conv(W[f'layers.{i}.adjust{j}'], t_pl, cin_planes=cp, act=L.ACT_LRELU, act_param=0.2, out_f32=chan_view(cur, dim, gc)))
                    else:
                        plan.conv(f32_view_conv(W[f'layers.{i}.adjust{j}'], t_pl, cin_planes=cp, res1=chan_view(cur, 0, C_), alpha=0.2, out_f32=chan_view(nxt, 0, C_)))
                ci ^= 1
            cur = cat[ci]
            norm('norm', chan_view(cur, 0, C_), C_, out_planes=n_pl)
            cp0 = (C_ + 7) // 8
            # conv_after_body(forward_features(x)) + conv_first(x) (arch.py:781): a 3x3 convolution, or nn.Identity (arch.py:731-732) -- the
            # latter as a 1x1 convolution with the identity matrix, whose epilogue adds conv_first's map and writes the planes the head reads
            plan.conv(ops.conv_params(W['conv_after_body' if self.resi == '1conv' else 'identity'], n_pl, H, Wd, cin_planes=cp0, res1=first, alpha=1.0, out=body_pl))
            pixelshuffle_head(plan, W, head, body_pl, cp0, H, Wd, y_out[bi : bi + 1], **final)
            plan.flush()

        for bi in range(nb):
            image(bi)
        return set_input
