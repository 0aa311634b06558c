"""SwinIR on the MI355X engine (reference module: ``resselt/archs/swinir/arch.py:735-1015``).

Tokens are pixels and never change layout: the f32 NCHW4c map is the residual stream, LayerNorm writes split planes,
every ``nn.Linear`` is a k1 convolution of the conv engine (GELU / residual adds in its epilogue), the attention core
runs in ``rsa_window_attention`` with roll / window partition / mask / relative-position bias as index arithmetic, and
the 1conv/3conv residual tails and the upsampling head are ordinary fused convolutions.

Weight re-layout at pack time (never per forward):
  * qkv rows are regrouped per head and zero-padded to 32 channels, q rows pre-multiplied by head_dim**-0.5;
    proj columns are padded the same way;
  * ``relative_position_bias_table[relative_position_index]`` is gathered once into accumulator-fragment order.
"""

from __future__ import annotations

import os

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, PF_F16
from ...engine.transformer import (HEAD_PAD, LayerPacker, ResidualTail, bias_fragments, bias_fragments16, head_macs, head_shapes, layernorm_on, mlp_block,
                                   mlp_block_fits, pack_head, reconstruction_head, regroup_proj, regroup_qkv, relative_position_index, shift_mask,
                                   tail_layers, tail_macs, tail_shapes)

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # resselt/archs/swinir/arch.py:788-790


def swinir_param_shapes(in_ch, out_ch, embed_dim, depths, num_heads, window, mlp_ratio, upscale, upsampler, resi, img_size, patch_norm=True):
    s = ParamShapes()
    buffers: dict = {}
    C_ = embed_dim
    hidden = int(C_ * mlp_ratio)

    s.conv('conv_first', C_, in_ch, 3)
    if patch_norm:
        s.norm('patch_embed.norm', C_)
    rp = relative_position_index(window)
    mask = None
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f'layers.{i}.residual_group.blocks.{j}'
            if j % 2 == 1:
                if mask is None:
                    mask = shift_mask(img_size, img_size, (window, window), (window // 2, window // 2))
                buffers[f'{b}.attn_mask'] = mask
            s.norm(f'{b}.norm1', C_)
            s[f'{b}.attn.relative_position_bias_table'] = ((2 * window - 1) ** 2, num_heads[i])
            buffers[f'{b}.attn.relative_position_index'] = rp
            s.linear(f'{b}.attn.qkv', 3 * C_, C_)
            s.linear(f'{b}.attn.proj', C_, C_)
            s.norm(f'{b}.norm2', C_)
            s.linear(f'{b}.mlp.fc1', hidden, C_)
            s.linear(f'{b}.mlp.fc2', C_, hidden)
        tail_shapes(s, f'layers.{i}.conv', C_, resi)
    s.norm('norm', C_)
    tail_shapes(s, 'conv_after_body', C_, resi)
    head_shapes(s, upsampler, C_, 64, out_ch, upscale)
    return s, buffers


class SwinIR(EngineModule):
    hyperparameters = {}
    # 'whole': one launch per block (csrc/swin_block_full.hip); 'halves': one launch per block half (csrc/swin_block.hip); False: the
    # layer-by-layer path (LayerNorm, Linear layers as k1 convolutions, rsa_window_attention).  The fused kernels take C <= 256,
    # <= 8 heads of <= 32 channels, window <= 8, hidden <= 512; other widths run layer by layer whatever this says.
    fused_blocks = 'whole'
    tail_slices = os.environ.get('RSA_SWIN_TAIL_SLICES', '0') != '0'  # 3conv tails: the C/4 -> C convolution as <= 64-channel slices on the ring. Correct
    # (the GPU suite passes with it) but 2 % SLOWER on C4 than the one chunk-barrier launch (profiles/r04_y_swin_tail_slices_ab.txt): off
    # 'mixed' (what 'auto' selects when every block runs as one fused launch): the transformer blocks and the convolution that closes each
    # residual group -- 95 % of the multiply-accumulates, all of them feeding the f32 residual stream through a LayerNorm -- run ONE fp16
    # product per multiply (weights, LayerNorm outputs, q / k / v, softmax probabilities, hidden activations rounded to 11 bits, f32
    # accumulation); the one-product block kernel keeps no lo images: 64 KB of LDS, two windows per CU.  The layers whose output reaches the
    # image at full amplitude run three products: conv_first and the reconstruction head in bf16 (the kernels of RRDBNet's tail),
    # conv_after_body in fp16 on the hi + lo output of the last LayerNorm.  One product everywhere ('fp16') measures 6-8e-4 on the
    # single-convolution heads (pixelshuffledirect, denoising); 'mixed' is pinned at <= 2e-4 on fp32 tensors by
    # tests/test_baseline_configs_gpu.py (C4, full depth) and test_swinir_gpu.py.  Models the fused kernels do not take keep 'bf16x3'.
    precisions = ('bf16x3', 'bf16', 'fp16', 'mixed')
    precision_table = {'mixed': (1, PF_F16)}

    @property
    def auto_precision(self) -> str:
        hidden = int(self.embed_dim * self.mlp_ratio)
        fused = self.fused_blocks == 'whole' and mlp_block_fits(self.embed_dim, hidden)
        fused = fused and all(h <= 8 and self.embed_dim // h <= HEAD_PAD for h in self.num_heads)
        return 'mixed' if fused else 'bf16x3'

    @staticmethod
    def layer_policy(name: str) -> tuple[int, int]:
        """(products, plane format of inputs and weights) of layer ``name`` (convolution or Linear) under 'mixed'."""
        if name == 'conv_first':
            return 3, PF_BF16
        if name.startswith('conv_after_body'):
            return 3, PF_F16
        if name.startswith('layers.'):
            return 1, PF_F16
        return 3, PF_BF16  # the reconstruction head

    def __init__(self, *, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, ape=False,
                 patch_norm=True, use_checkpoint=False, upscale=1, img_range=1.0, upsampler='', resi_connection='1conv',
                 start_unshuffle=1) -> None:  # fmt: skip
        super().__init__()
        if patch_size != 1 or ape or not qkv_bias or qk_scale is not None:
            raise NotImplementedError('SwinIR engine supports patch_size=1, ape=False, qkv_bias=True, default qk scale (what the loader builds)')
        if start_unshuffle != 1:
            raise NotImplementedError('start_unshuffle > 1 cannot load in the reference either (SURVEY.md §4 defect 6)')
        if window_size > 8:
            raise NotImplementedError('window_size must be <= 8 (64 tokens per window)')
        if min(img_size, img_size) <= window_size:
            raise NotImplementedError('img_size <= window_size changes the block geometry; not supported')
        depths, num_heads = list(depths), list(num_heads)
        if any(embed_dim % h or embed_dim // h > HEAD_PAD for h in num_heads):
            raise NotImplementedError('head_dim must divide embed_dim and be <= 32')
        if embed_dim % 4:
            raise NotImplementedError('embed_dim must be a multiple of 4')
        self.in_chans, self.out_chans = in_chans, in_chans
        self.embed_dim, self.depths, self.num_heads = embed_dim, depths, num_heads
        self.window_size, self.mlp_ratio = window_size, mlp_ratio
        self.upscale, self.img_range, self.upsampler = upscale, img_range, upsampler
        self.resi, self.patch_norm, self.img_size = resi_connection, patch_norm, img_size
        shapes, buffers = swinir_param_shapes(in_chans, in_chans, embed_dim, depths, num_heads, window_size, mlp_ratio, upscale, upsampler,
                                              resi_connection, img_size, patch_norm)  # fmt: skip
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device) for k, v in self.state_dict().items()}
        pk = LayerPacker(sd, device, products, self.layer_policy)
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln

        def resi_conv(name):
            for layer in tail_layers(name, self.resi):
                conv(layer)
            if self.resi == '3conv' and self.tail_slices:
                # Round 4: the last convolution of a 3conv tail (C/4 -> C, e.g. 60 -> 240) as output-channel SLICES of at most 64 channels: each
                # slice has whole 32-channel input chunks and 33..64 output channels, i.e. it takes the ring schedule (the whole layer ran the
                # chunk-barrier kernel: 0.82 ms per 1024^2 map; the four ring launches with their generic f32-residual epilogues take longer: profiles/r04_y_*).  One image per launch list only: a
                # slice of an f32 map is a channel view, contiguous for one image.
                w, b = sd[f'{name}.4.weight'], sd.get(f'{name}.4.bias')
                prod, fmt = pk.policy(f'{name}.4')
                for k, c0 in enumerate(range(0, w.shape[0], 64)):
                    W[f'{name}.4.s{k}'] = ops.ConvWeights.from_oihw(w[c0 : c0 + 64], None if b is None else b[c0 : c0 + 64], prod, device=device, fmt=fmt)

        conv('conv_first')
        if self.patch_norm:
            ln('patch_embed.norm')
        for i, depth in enumerate(self.depths):
            heads = self.num_heads[i]
            for j in range(depth):
                b = f'layers.{i}.residual_group.blocks.{j}'
                ln(f'{b}.norm1')
                ln(f'{b}.norm2')
                wq, bq = regroup_qkv(sd[f'{b}.attn.qkv.weight'], sd[f'{b}.attn.qkv.bias'], heads)
                lin(f'{b}.attn.qkv', wq, bq)
                lin(f'{b}.attn.proj', regroup_proj(sd[f'{b}.attn.proj.weight'], heads), sd[f'{b}.attn.proj.bias'], cin_planes=heads * HEAD_PAD // 8)
                lin(f'{b}.mlp.fc1')
                lin(f'{b}.mlp.fc2')
                W[f'{b}.bias_frag'] = bias_fragments(sd[f'{b}.attn.relative_position_bias_table'], sd[f'{b}.attn.relative_position_index'],
                                                     self.window_size)  # fmt: skip
                W[f'{b}.bias_frag16'] = bias_fragments16(sd[f'{b}.attn.relative_position_bias_table'], sd[f'{b}.attn.relative_position_index'],
                                                         self.window_size)  # fmt: skip
            resi_conv(f'layers.{i}.conv')
        ln('norm')
        resi_conv('conv_after_body')
        pack_head(pk)
        mean = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=device)
        W['mean'] = mean
        check_fp16_range(W.values())
        return W

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per (window-padded) input pixel: convs, Linear layers and the two attention contractions."""
        C_, w = self.embed_dim, self.window_size
        hidden = int(C_ * self.mlp_ratio)
        nblocks = sum(self.depths)
        macs = 9 * self.in_chans * C_
        macs += nblocks * (3 * C_ * C_ + C_ * C_ + 2 * C_ * hidden + 2 * w * w * C_)
        macs += (len(self.depths) + 1) * tail_macs(C_, self.resi)
        return macs + head_macs(self.upsampler, C_, 64, self.out_chans, self.upscale)

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, h0, w0 = x_shape
        if c != self.in_chans:
            raise RuntimeError(f'model expects {self.in_chans} input channels, got {c}')
        win = self.window_size
        H, Wd = h0 + (win - h0 % win) % win, w0 + (win - w0 % win) % win
        if H - h0 >= h0 or Wd - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to a multiple of the window size')
        C_, s = self.embed_dim, self.upscale
        hidden = int(C_ * self.mlp_ratio)
        with_lo = products == 3
        mixed = products.name == 'mixed'
        wide = with_lo or mixed  # buffers read by a three-product layer under 'mixed' keep hi + lo
        head_fmt = PF_BF16 if mixed else plan.fmt  # conv_first and the reconstruction head: bf16 planes under 'mixed'
        cp = (C_ + 7) // 8
        dev = plan.device

        x_pl = plan.planes(n, (c + 7) // 8, H, Wd, wide, head_fmt)
        mean = W['mean']

        def set_input(x):
            # check_image_size (reflect pad to the window multiple) and (x - mean) * img_range, fused (arch.py:964-967)
            ops.nchw_to_planes(x, x_pl, mean, self.img_range)

        first = plan.f32map(n, C_, H, Wd)
        pool = [plan.f32map(n, C_, H, Wd) for _ in range(4)]
        a_pl = plan.planes(n, cp, H, Wd, wide)  # LayerNorm output / conv input
        max_heads = max(self.num_heads)

        def can_fuse(heads):
            return self.fused_blocks and mlp_block_fits(C_, hidden) and heads <= 8 and C_ // heads <= HEAD_PAD

        if products.name in ('fp16', 'mixed') and not (self.fused_blocks == 'whole' and all(can_fuse(h) for h in self.num_heads)):
            raise NotImplementedError("SwinIR 'fp16' / 'mixed' need every block on the whole-block kernel (fused_blocks = 'whole', C <= 256, <= 8 heads of <= 32 "
                                      "channels, hidden <= 512); use precision 'bf16x3' or 'bf16'")  # fmt: skip
        if all(can_fuse(h) for h in self.num_heads):
            qkv_pl = o_pl = hid_pl = None  # nothing between the residual stream and itself leaves the chip
        else:
            qkv_pl = plan.planes(n, 3 * max_heads * HEAD_PAD // 8, H, Wd, with_lo)
            o_pl = plan.planes(n, max_heads * HEAD_PAD // 8, H, Wd, with_lo)
            hid_pl = plan.planes(n, (hidden + 7) // 8, H, Wd, with_lo)
        body_pl = plan.planes(n, cp, H, Wd, with_lo)  # the last block of a residual group -> that group's convolution
        head_pl = plan.planes(n, cp, H, Wd, wide, head_fmt) if mixed else body_pl  # conv_after_body -> the reconstruction head
        tail = ResidualTail(plan, W, self.resi, n, H, Wd, C_, wide)
        norm = layernorm_on(plan, W, n, H, Wd, C_)

        def attention(name, heads, shift):
            ap = L.WindowAttnParams()
            ap.batch, ap.H, ap.W, ap.heads, ap.window, ap.shift, ap.products = n, H, Wd, heads, win, shift, products
            qkv_pl.bind(ap, 'qkv')
            ap.bias_frag = W[f'{name}.bias_frag'].data_ptr()
            o_pl.bind(ap, 'out')
            plan.launch('rsa_window_attention', ap)

        def attn_block(name, heads, shift, x_f32, out_f32):
            """norm1 -> qkv -> window attention -> proj -> + shortcut in one launch (arch.py:295-330)."""
            g, be = W[f'{name}.norm1']
            qkv, proj = W[f'{name}.attn.qkv'], W[f'{name}.attn.proj']
            ap = L.SwinAttnBlockParams()
            ap.batch, ap.H, ap.W, ap.C, ap.heads, ap.window, ap.shift, ap.products, ap.eps = n, H, Wd, C_, heads, win, shift, products, 1e-5
            ap.x, ap.gamma, ap.beta = x_f32.data_ptr(), g.data_ptr(), be.data_ptr()
            ap.wqkv, ap.bqkv = qkv.packed_for(0).data_ptr(), qkv.bias.data_ptr()
            ap.bias_frag16 = W[f'{name}.bias_frag16'].data_ptr()
            ap.wproj, ap.bproj = proj.packed_for(0).data_ptr(), proj.bias.data_ptr()
            ap.out = out_f32.data_ptr()
            plan.launch('rsa_swin_attn_block', ap)

        def whole_block(name, heads, shift, x_f32, out_f32, out_planes=None):
            """The whole block in one launch (arch.py:295-335; csrc/swin_block_full.hip): x1 never leaves the chip."""
            g1, be1 = W[f'{name}.norm1']
            g2, be2 = W[f'{name}.norm2']
            qkv, proj, fc1, fc2 = (W[f'{name}.{k}'] for k in ('attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2'))
            bp = L.SwinBlockParams()
            bp.batch, bp.H, bp.W, bp.C, bp.heads, bp.window, bp.shift, bp.hidden, bp.products, bp.eps = n, H, Wd, C_, heads, win, shift, hidden, products, 1e-5
            bp.x, bp.gamma1, bp.beta1, bp.gamma2, bp.beta2 = x_f32.data_ptr(), g1.data_ptr(), be1.data_ptr(), g2.data_ptr(), be2.data_ptr()
            bp.wqkv, bp.bqkv = qkv.packed_for(0).data_ptr(), qkv.bias.data_ptr()
            bp.bias_frag16 = W[f'{name}.bias_frag16'].data_ptr()
            bp.wproj, bp.bproj = proj.packed_for(0).data_ptr(), proj.bias.data_ptr()
            bp.w1, bp.b1, bp.w2, bp.b2 = fc1.packed_for(0).data_ptr(), fc1.bias.data_ptr(), fc2.packed_for(0).data_ptr(), fc2.bias.data_ptr()
            bp.out = out_f32.data_ptr()
            bp.fmt = plan.fmt
            if out_planes is not None:
                out_planes.bind(bp, 'out')
            tokens = n * H * Wd
            meta = dict(kernel=f'rsa::swin_block_kernel<{int(products)},{"f16" if plan.fmt == PF_F16 else "bf16"}> (whole Swin block)', products=int(products),
                        flop=2.0 * tokens * (4 * C_ * C_ + 2 * C_ * hidden + 2 * win * win * C_),  # qkv + proj, the MLP, QK^T and PV
                        bytes=2.0 * tokens * C_ * 4 + (0 if out_planes is None else tokens * C_ * 2.0 * (2 if out_planes.lo is not None else 1)))  # fmt: skip
            plan.launch('rsa_swin_block', bp, meta=meta)

        def mlp(name, x_f32, out_f32, out_planes=None):
            mlp_block(plan, W[f'{name}.norm2'], W[f'{name}.mlp.fc1'], W[f'{name}.mlp.fc2'], n, H, Wd, C_, hidden, products, x_f32, out_f32, out_planes)

        def resi_conv(name, src_planes, res, out_f32=None, out_planes=None):
            """1conv / 3conv tail (arch.py:562-574) + the residual add that follows it."""
            if n == 1 and f'{name}.4.s0' in W and C_ % 8 == 0:  # (`tail_slices`: the last convolution in <= 64-channel slices)
                q4 = tail.squeeze(name, src_planes)
                for k, c0 in enumerate(range(0, C_, 64)):
                    cw = min(64, C_ - c0)
                    plan.conv(ops.conv_params(W[f'{name}.4.s{k}'], q4, H, Wd, res1=res[:, c0 // 4 : (c0 + cw) // 4], alpha=1.0,
                                              out_f32=None if out_f32 is None else out_f32[:, c0 // 4 : (c0 + cw) // 4],
                                              out=out_planes, out_plane_off=c0 // 8))  # fmt: skip
            else:
                tail(name, src_planes, res, out_f32, out_planes)

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
            rstb_in = cur
            for j in range(depth):
                b = f'layers.{i}.residual_group.blocks.{j}'
                shift = 0 if j % 2 == 0 else win // 2
                last = j == depth - 1
                x1 = free.pop()
                if can_fuse(heads) and self.fused_blocks == 'whole':
                    x2 = free.pop()
                    whole_block(b, heads, shift, cur, x2, body_pl if last else None)
                elif can_fuse(heads):
                    attn_block(b, heads, shift, cur, x1)
                    x2 = free.pop()
                    mlp(b, x1, x2, body_pl if last else None)
                else:
                    norm(f'{b}.norm1', cur, out_planes=a_pl)
                    plan.conv(ops.conv_params(W[f'{b}.attn.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                    attention(b, heads, shift)
                    plan.conv(ops.conv_params(W[f'{b}.attn.proj'], o_pl, H, Wd, cin_planes=hp, res1=cur, alpha=1.0, out_f32=x1))
                    norm(f'{b}.norm2', x1, out_planes=a_pl)
                    plan.conv(ops.conv_params(W[f'{b}.mlp.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
                    x2 = free.pop()
                    plan.conv(ops.conv_params(W[f'{b}.mlp.fc2'], hid_pl, H, Wd, cin_planes=(hidden + 7) // 8, res1=x1, alpha=1.0, out_f32=x2,
                                              out=body_pl if last else None))  # fmt: skip
                if cur is not rstb_in and cur is not first:
                    free.append(cur)
                free.append(x1)
                cur = x2
            out = free.pop()
            resi_conv(f'layers.{i}.conv', body_pl, rstb_in, out_f32=out)
            if rstb_in is not first:
                free.append(rstb_in)
            if cur is not rstb_in:
                free.append(cur)
            cur = out
        norm('norm', cur, out_planes=a_pl)
        resi_conv('conv_after_body', a_pl, first, out_planes=head_pl)  # + conv_first output (arch.py:988)
        body_pl = head_pl  # (the head reads conv_after_body's output from here on)
        with_lo, plan_fmt = wide, plan.fmt
        plan.fmt = head_fmt  # buffers of the head

        y_out = plan.output((n, self.out_chans, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        # the last store: x / img_range + mean (arch.py:1013); the denoising / JPEG artefact heads add the caller's own input (arch.py:1007-1010)
        reconstruction_head(plan, W, self.upsampler, body_pl, cp, n, H, Wd, s, with_lo, y_out, 1.0 / self.img_range, mean, (x_shape, dtype))
        plan.fmt = plan_fmt
        return set_input
