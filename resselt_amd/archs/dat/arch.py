"""DAT (Dual Aggregation Transformer) on the MI355X engine -- drop-in for ``resselt/archs/dat/arch.py:828-990`` in eval mode.

Tokens are pixels.  The residual stream is an f32 map, every Linear layer is a k1 launch of the convolution kernels, and the
rest of the block runs on the kernels of ``csrc/dat.hip``:

  DSTB (even blocks, arch.py:270-513)   LN -> qkv -> 2 x rect-window attention (8x32 and 32x8 on the two channel halves, shifted on
                                        every second one) -> depthwise conv(v) -> channel gate -> AIM combine -> proj (+ residual)
  DCTB (odd blocks,  arch.py:516-612)   LN -> qkv -> channel attention: Gram matrix over all tokens -> softmax -> packed 1x1
                                        weights -> attn @ v as one more conv launch -> depthwise conv(v) -> gate -> AIM -> proj
  SGFN (arch.py:42-101)                 LN -> fc1 + GELU -> per-pixel LN statistics of the second half -> depthwise conv of the
                                        normalised half, multiplied by the first half -> fc2 (+ residual)

Attention-side maps use the head-padded channel layout (head h = channels [32h, 32h+32)); every weight that touches them is
permuted once at pack time.  BatchNorm is folded with its running statistics (the reference module straight from the loader is
in training mode, where DropPath is random and BatchNorm uses batch statistics; inference callers use ``.eval()``).
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, PF_F16, Planes
from ...engine.transformer import (HEAD_PAD, LayerPacker, ResidualTail, attn_tiles, bias_fragments_qk, branch_geometry, dwconv3x3, head_macs, head_shapes,
                                   layernorm_on, pack_head, pad_heads, plane_stats, reconstruction_head, rect_attention, regroup_proj, regroup_qkv,
                                   relative_position_index, shift_mask, tail_layers, tail_macs, tail_shapes)

RGB_MEAN = (0.4488, 0.4371, 0.4040)  # arch.py:879
BN_EPS = 1e-5

# names this module exported before the shared helpers moved to engine/transformer.py (attn_tiles, branch_geometry and pad_heads are imported above)
bias_fragments = bias_fragments_qk


def is_shifted(rg_idx: int, b_idx: int) -> bool:  # arch.py:312, 453
    return (rg_idx % 2 == 0 and b_idx > 0 and (b_idx - 2) % 4 == 0) or (rg_idx % 2 != 0 and b_idx % 4 == 0)


def rpe_buffers(hs: int, ws: int):
    """``rpe_biases`` and ``relative_position_index`` buffers of one Spatial_Attention (arch.py:193-211)."""
    bh, bw = torch.arange(1 - hs, hs), torch.arange(1 - ws, ws)
    biases = torch.stack(torch.meshgrid([bh, bw], indexing='ij')).flatten(1).transpose(0, 1).contiguous().float()
    return biases, relative_position_index(hs, ws)


def shift_masks(H: int, W: int, split, shift):
    """The registered ``attn_mask_0/1`` buffers (arch.py:336-411); kept for state_dict parity, the kernel derives the mask itself."""
    return [shift_mask(H, W, branch_geometry(split, idx), branch_geometry(shift, idx)) for idx in (0, 1)]


def pad_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    out = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
    out[: t.shape[0]] = t.to(torch.float32)
    return out.contiguous()


def dat_param_shapes(in_chans, embed_dim, split_size, depth, num_heads, expansion_factor, qkv_bias, upscale, resi, upsampler, img_size):
    s = ParamShapes()
    buffers: dict = {}
    C_ = embed_dim
    hidden = int(C_ * expansion_factor)
    shift_size = [split_size[0] // 2, split_size[1] // 2]

    def bn(name, c):
        s.norm(name, c)
        buffers[f'{name}.running_mean'] = torch.zeros(c)
        buffers[f'{name}.running_var'] = torch.ones(c)
        buffers[f'{name}.num_batches_tracked'] = torch.tensor(0, dtype=torch.int64)

    def dw(name, c):
        s[f'{name}.weight'] = (c, 1, 3, 3)
        s[f'{name}.bias'] = (c,)

    def aim(name):
        dw(f'{name}.dwconv.0', C_)
        bn(f'{name}.dwconv.1', C_)
        s.conv(f'{name}.channel_interaction.1', C_ // 8, C_, 1)
        bn(f'{name}.channel_interaction.2', C_ // 8)
        s.conv(f'{name}.channel_interaction.4', C_, C_ // 8, 1)
        s.conv(f'{name}.spatial_interaction.0', C_ // 16, C_, 1)
        bn(f'{name}.spatial_interaction.1', C_ // 16)
        s.conv(f'{name}.spatial_interaction.3', 1, C_ // 16, 1)

    pos_dim = ((C_ // 2) // 4) // 4
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
            else:
                s[f'{b}.attn.temperature'] = (heads, 1, 1)
                s.linear(f'{b}.attn.qkv', 3 * C_, C_, qkv_bias)
                s.linear(f'{b}.attn.proj', C_, C_)
            aim(f'{b}.attn')
            s.linear(f'{b}.ffn.fc1', hidden, C_)
            s.norm(f'{b}.ffn.sg.norm', hidden // 2)
            dw(f'{b}.ffn.sg.conv', hidden // 2)
            s.linear(f'{b}.ffn.fc2', C_, hidden // 2)
            s.norm(f'{b}.norm2', C_)
        tail_shapes(s, f'layers.{i}.conv', C_, resi)
    s.norm('norm', C_)
    tail_shapes(s, 'conv_after_body', C_, resi)
    head_shapes(s, upsampler, C_, 64, in_chans, upscale)
    return s, buffers


class DAT(EngineModule):
    hyperparameters = {}
    # 'mixed' (what 'auto' selects).  Round 4: the WHOLE transformer body runs on fp16 hi planes in one product -- qkv, proj, fc1, fc2, the
    # rectangular-window attention (`rect_attention_kernel<1, T, f16>`), the channel attention's Gram matrix and its `attn @ v` (the weight
    # blob is written in fp16), the depthwise convolutions, the AIM, the spatial gate (their descriptors carry the plane format) -- as HAT and
    # DRCT have done since round 3.  The residual stream stays an f32 map; the 3x3 convolutions of the residual groups, conv_first,
    # conv_after_body and the reconstruction head keep three bf16 products.  (Round 3: only qkv and fc1, the layers a LayerNorm feeds.)
    auto_precision = 'mixed'
    precisions = ('bf16x3', 'bf16', 'mixed')
    precision_table = {'mixed': (3, PF_BF16)}

    @staticmethod
    def layer_policy(name: str) -> tuple[int, int]:
        """(products, plane format of inputs and weights) of layer ``name`` under 'mixed'."""
        return (1, PF_F16) if name.endswith(('.attn.qkv', '.attn.proj', '.ffn.fc1', '.ffn.fc2')) else (3, PF_BF16)

    def __init__(self, *, img_size=64, in_chans=3, embed_dim=180, split_size=(8, 32), depth=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6),
                 expansion_factor=2.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_chk=False,
                 upscale=4, img_range=1.0, resi_connection='1conv', upsampler='pixelshuffle') -> None:  # fmt: skip
        super().__init__()
        split_size, depth, num_heads = list(split_size), list(depth), list(num_heads)
        if qk_scale is not None:
            raise NotImplementedError('DAT engine supports the default qk scale (what the loader builds)')
        if upsampler not in ('pixelshuffle', 'pixelshuffledirect'):
            raise NotImplementedError(f'upsampler {upsampler!r} is not a DAT upsampler')
        if split_size[0] * split_size[1] > 256 or min(split_size) < 2:
            raise NotImplementedError('split_size must hold 4..256 tokens with both sides >= 2')
        if embed_dim % 4 or any(h % 2 or embed_dim % h or embed_dim // h > HEAD_PAD for h in num_heads):
            raise NotImplementedError('embed_dim must be a multiple of 4, heads even, head_dim <= 32')
        if not 1 <= embed_dim // 16 <= 16:
            raise NotImplementedError('embed_dim // 16 (spatial-interaction width) must be in 1..16')
        hidden = int(embed_dim * expansion_factor)
        if hidden % 2:
            raise NotImplementedError('the SGFN hidden width must be even')
        self.in_chans, self.embed_dim, self.split_size, self.depth, self.num_heads = in_chans, embed_dim, split_size, depth, num_heads
        self.hidden, self.qkv_bias, self.upscale, self.img_range = hidden, qkv_bias, upscale, img_range
        self.resi, self.upsampler, self.img_size = resi_connection, upsampler, img_size
        shapes, buffers = dat_param_shapes(in_chans, embed_dim, split_size, depth, num_heads, expansion_factor, qkv_bias, upscale, resi_connection,
                                           upsampler, img_size)  # fmt: skip
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device) for k, v in self.state_dict().items()}
        C_ = self.embed_dim
        pk = LayerPacker(sd, device, products, self.layer_policy)
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln

        def f32(t):
            return t.to(torch.float32).contiguous()

        def resi_conv(name):
            for layer in tail_layers(name, self.resi):
                conv(layer)

        def bn_fold(name):
            """(scale, shift) of an eval-mode BatchNorm: y = x * scale + shift."""
            s = f32(sd[f'{name}.weight']) / torch.sqrt(f32(sd[f'{name}.running_var']) + BN_EPS)
            return s, f32(sd[f'{name}.bias']) - f32(sd[f'{name}.running_mean']) * s

        def pos_bias(a):
            """DynamicPosBias (residual=False, arch.py:104-143) on rpe_biases, gathered to [heads, N, N] (arch.py:247-252)."""
            F = torch.nn.functional
            pos = F.linear(f32(sd[f'{a}.rpe_biases']), f32(sd[f'{a}.pos.pos_proj.weight']), f32(sd[f'{a}.pos.pos_proj.bias']))
            for k in ('pos1', 'pos2', 'pos3'):
                g = f32(sd[f'{a}.pos.{k}.0.weight'])
                pos = F.layer_norm(pos, (g.shape[0],), g, f32(sd[f'{a}.pos.{k}.0.bias']), 1e-5)
                pos = F.linear(F.relu(pos), f32(sd[f'{a}.pos.{k}.2.weight']), f32(sd[f'{a}.pos.{k}.2.bias']))
            idx = sd[f'{a}.relative_position_index'].long()
            n = idx.shape[0]
            return pos[idx.reshape(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()

        def aim(a, heads):
            s, t = bn_fold(f'{a}.dwconv.1')
            w = f32(sd[f'{a}.dwconv.0.weight']).reshape(C_, 9) * s[:, None]
            W[f'{a}.dw'] = (pad_heads(w, heads), pad_heads(f32(sd[f'{a}.dwconv.0.bias']) * s + t, heads))
            s, t = bn_fold(f'{a}.channel_interaction.2')
            w1 = f32(sd[f'{a}.channel_interaction.1.weight']).reshape(-1, C_) * s[:, None]
            b1 = f32(sd[f'{a}.channel_interaction.1.bias']) * s + t
            w2 = f32(sd[f'{a}.channel_interaction.4.weight']).reshape(C_, -1)
            W[f'{a}.ci'] = (pad_heads(w1, heads, dim=1), b1.contiguous(), pad_heads(w2, heads), pad_heads(f32(sd[f'{a}.channel_interaction.4.bias']), heads))
            s, t = bn_fold(f'{a}.spatial_interaction.1')
            w1 = f32(sd[f'{a}.spatial_interaction.0.weight']).reshape(-1, C_) * s[:, None]
            b1 = f32(sd[f'{a}.spatial_interaction.0.bias']) * s + t
            W[f'{a}.si'] = (pad_heads(w1, heads, dim=1), b1.contiguous(), f32(sd[f'{a}.spatial_interaction.3.weight']).reshape(-1),
                            float(sd[f'{a}.spatial_interaction.3.bias'].float().item()))  # fmt: skip

        half = self.hidden // 2
        P1 = (half + 7) // 8
        conv('conv_first')
        ln('before_RG.1')
        for i, d in enumerate(self.depth):
            heads = self.num_heads[i]
            for j in range(d):
                b = f'layers.{i}.blocks.{j}'
                ln(f'{b}.norm1')
                ln(f'{b}.norm2')
                spatial = j % 2 == 0
                wq, bq = regroup_qkv(sd[f'{b}.attn.qkv.weight'], sd.get(f'{b}.attn.qkv.bias'), heads, scale_q=spatial)
                lin(f'{b}.attn.qkv', wq, bq)
                lin(f'{b}.attn.proj', regroup_proj(sd[f'{b}.attn.proj.weight'], heads), sd[f'{b}.attn.proj.bias'], cin_planes=heads * HEAD_PAD // 8)
                if spatial:
                    for idx in (0, 1):
                        W[f'{b}.attn.bias{idx}'] = bias_fragments_qk(pos_bias(f'{b}.attn.attns.{idx}'))
                else:
                    W[f'{b}.attn.temperature'] = f32(sd[f'{b}.attn.temperature']).reshape(-1)
                aim(f'{b}.attn', heads)
                # fc1 rows: x1 = rows [0, half) on planes [0, P1), x2 = rows [half, 2*half) on planes [P1, 2*P1)
                w1 = torch.zeros((2 * P1 * 8, C_), dtype=torch.float32, device=device)
                b1 = torch.zeros((2 * P1 * 8,), dtype=torch.float32, device=device)
                fw, fb = f32(sd[f'{b}.ffn.fc1.weight']), f32(sd[f'{b}.ffn.fc1.bias'])
                w1[:half], w1[P1 * 8 : P1 * 8 + half] = fw[:half], fw[half:]
                b1[:half], b1[P1 * 8 : P1 * 8 + half] = fb[:half], fb[half:]
                lin(f'{b}.ffn.fc1', w1, b1)
                lin(f'{b}.ffn.fc2')
                W[f'{b}.ffn.sg'] = (pad_rows(f32(sd[f'{b}.ffn.sg.conv.weight']).reshape(half, 9), P1 * 8), pad_rows(f32(sd[f'{b}.ffn.sg.conv.bias']), P1 * 8),
                                    pad_rows(f32(sd[f'{b}.ffn.sg.norm.weight']), P1 * 8), pad_rows(f32(sd[f'{b}.ffn.sg.norm.bias']), P1 * 8))  # fmt: skip
            resi_conv(f'layers.{i}.conv')
        ln('norm')
        resi_conv('conv_after_body')
        pack_head(pk)
        check_fp16_range(W.values())
        W['mean'] = torch.tensor(RGB_MEAN if self.in_chans == 3 else [0.0] * self.in_chans, dtype=torch.float32, device=device)
        return W

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per input pixel (convs, Linear layers, both attention kinds, depthwise convs; AIM gates neglected)."""
        C_, hid = self.embed_dim, self.hidden
        ntok = self.split_size[0] * self.split_size[1]
        macs = 9 * self.in_chans * C_
        resi = tail_macs(C_, self.resi)
        for i, d in enumerate(self.depth):
            hd = C_ // self.num_heads[i]
            for j in range(d):
                macs += 3 * C_ * C_ + C_ * C_ + 9 * C_  # qkv, proj, depthwise conv on v
                macs += 2 * ntok * C_ if j % 2 == 0 else 2 * hd * C_  # QK^T + PV, or Gram + attn @ v
                macs += C_ * hid + 9 * (hid // 2) + (hid // 2) * C_  # SGFN
            macs += resi
        return macs + resi + head_macs(self.upsampler, C_, 64, self.in_chans, self.upscale)

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, H, Wd = x_shape
        if c != self.in_chans:
            raise RuntimeError(f'model expects {self.in_chans} input channels, got {c}')
        C_, s = self.embed_dim, self.upscale
        with_lo = products == 3
        cp = (C_ + 7) // 8
        half = self.hidden // 2
        P1 = (half + 7) // 8
        dev = plan.device
        lib = L.load()
        max_heads = max(self.num_heads)
        hp_max = max_heads * HEAD_PAD // 8

        x_pl = plan.planes(n, (c + 7) // 8, H, Wd, with_lo)
        mean = W['mean']

        def set_input(x):
            ops.nchw_to_planes(x, x_pl, mean, self.img_range)  # (x - mean) * img_range (arch.py:975-976)

        first = plan.f32map(n, C_, H, Wd)
        pool = [plan.f32map(n, C_, H, Wd) for _ in range(4)]
        mixed = products.name == 'mixed'
        body_kw = dict(with_lo=False, fmt=PF_F16) if mixed else dict(with_lo=with_lo)  # the transformer body: fp16 hi planes under 'mixed'
        bprod = 1 if mixed else int(products)  # matrix products of the body's attention kernels
        bfmt = PF_F16 if mixed else products.fmt
        a_pl = plan.planes(n, cp, H, Wd, **body_kw)  # norm1 / norm2 -> qkv / fc1
        n_pl = plan.planes(n, cp, H, Wd, with_lo) if mixed else a_pl  # the last LayerNorm -> conv_after_body (three products)
        qkv_pl = plan.planes(n, 3 * hp_max, H, Wd, **body_kw)
        att_pl = plan.planes(n, hp_max, H, Wd, **body_kw)
        conv_pl = plan.planes(n, hp_max, H, Wd, **body_kw)
        comb_pl = plan.planes(n, hp_max, H, Wd, **body_kw)
        hid_pl = plan.planes(n, 2 * P1, H, Wd, **body_kw)
        gate_pl = plan.planes(n, P1, H, Wd, **body_kw)
        body_pl = plan.planes(n, cp, H, Wd, with_lo)
        resi_conv = ResidualTail(plan, W, self.resi, n, H, Wd, C_, with_lo)
        stats = torch.empty((n, H * Wd, 2), dtype=torch.float32, device=dev)
        gate = torch.empty((n, max_heads * HEAD_PAD), dtype=torch.float32, device=dev)
        ws_gate = torch.empty((max(int(lib.rsa_channel_gate_workspace_bytes(n, H, Wd, hp_max)), 16) // 4,), dtype=torch.float32, device=dev)
        has_dctb = any(d >= 2 for d in self.depth)
        ws_attn = torch.empty((max(int(lib.rsa_channel_attn_workspace_bytes(n, H, Wd, max_heads)), 16) // 4,), dtype=torch.float32, device=dev)
        zero_bias = torch.zeros((max_heads * HEAD_PAD,), dtype=torch.float32, device=dev)
        plan.keep += [stats, gate, ws_gate, ws_attn, zero_bias]
        wdyn = {}
        if has_dctb:
            for heads in sorted({h for h, d in zip(self.num_heads, self.depth) if d >= 2}):
                blob = int(lib.rsa_packed_weight_bytes(heads * HEAD_PAD, heads * 4, 1, bprod)) // 2
                wdyn[heads] = torch.zeros((n, blob), dtype=torch.bfloat16, device=dev)  # off-diagonal blocks stay zero forever
                plan.keep.append(wdyn[heads])

        norm = layernorm_on(plan, W, n, H, Wd, C_)

        def channel_attention(b, heads):
            hp = heads * 4
            cpar = L.ChannelAttnParams()
            cpar.batch, cpar.H, cpar.W, cpar.heads, cpar.head_dim, cpar.products = n, H, Wd, heads, C_ // heads, bprod
            cpar.fmt = bfmt
            cpar.q_hi, cpar.q_lo = qkv_pl.hi_ptr(0), qkv_pl.lo_ptr(0)
            cpar.k_hi, cpar.k_lo = qkv_pl.hi_ptr(hp), qkv_pl.lo_ptr(hp)
            cpar.plane_stride, cpar.batch_stride = qkv_pl.plane_stride, qkv_pl.batch_stride
            cpar.temperature = W[f'{b}.attn.temperature'].data_ptr()
            cpar.workspace, cpar.w_packed = ws_attn.data_ptr(), wdyn[heads].data_ptr()
            plan.launch('rsa_channel_attention_weights', cpar, kernels=2)
            for bi in range(n):  # attn @ v: the weights differ per image
                wts = ops.ConvWeights(wdyn[heads][bi], zero_bias, heads * HEAD_PAD, heads * HEAD_PAD, hp, 1, bprod, fmt=bfmt)
                src = Planes(qkv_pl.hi[bi : bi + 1], None if qkv_pl.lo is None else qkv_pl.lo[bi : bi + 1])
                dst = Planes(att_pl.hi[bi : bi + 1], None if att_pl.lo is None else att_pl.lo[bi : bi + 1])
                plan.conv(ops.conv_params(wts, src, H, Wd, in_plane0=2 * hp, cin_planes=hp, out=dst))

        def channel_gate(a, src, heads):
            w1, b1, w2, b2 = W[f'{a}.ci']
            gp = L.ChannelGateParams()
            gp.batch, gp.H, gp.W, gp.planes, gp.hidden = n, H, Wd, heads * 4, w1.shape[0]
            gp.fmt = src.fmt
            src.bind(gp, 'in')
            gp.w1, gp.b1, gp.w2, gp.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
            gp.workspace, gp.gate = ws_gate.data_ptr(), gate.data_ptr()
            plan.launch('rsa_channel_gate', gp, kernels=2)

        def aim_combine(a, heads, mode):
            w1, b1, w2, b2 = W[f'{a}.si']
            ap = L.AimParams()
            ap.batch, ap.H, ap.W, ap.planes, ap.hidden, ap.mode = n, H, Wd, heads * 4, w1.shape[0], mode
            ap.fmt = att_pl.fmt
            att_pl.bind(ap, 'att')
            conv_pl.bind(ap, 'conv')
            ap.gate, ap.w1, ap.b1, ap.w2, ap.b2 = gate.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2
            comb_pl.bind(ap, 'out')
            plan.launch('rsa_aim_combine', ap)

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
                plan.conv(ops.conv_params(W[f'{a}.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                if j % 2 == 0:
                    rect_attention(plan, qkv_pl, att_pl, [W[f'{a}.bias{idx}'] for idx in (0, 1)], n, H, Wd, self.split_size, heads, is_shifted(i, j), bprod, bfmt)
                    dwconv3x3(plan, W[f'{a}.dw'], qkv_pl, 2 * hp, hp, conv_pl, act=L.ACT_GELU)
                    channel_gate(a, conv_pl, heads)
                    aim_combine(a, heads, 0)
                else:
                    channel_attention(b, heads)
                    dwconv3x3(plan, W[f'{a}.dw'], qkv_pl, 2 * hp, hp, conv_pl, act=L.ACT_GELU)
                    channel_gate(a, att_pl, heads)
                    aim_combine(a, heads, 1)
                x1 = free.pop()
                plan.conv(ops.conv_params(W[f'{a}.proj'], comb_pl, H, Wd, cin_planes=hp, res1=cur, alpha=1.0, out_f32=x1))
                norm(f'{b}.norm2', x1, out_planes=a_pl)
                plan.conv(ops.conv_params(W[f'{b}.ffn.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
                sgw, sgb, sgg, sgbeta = W[f'{b}.ffn.sg']
                plane_stats(plan, hid_pl, P1, half, stats)
                dwconv3x3(plan, (sgw, sgb), hid_pl, P1, P1, gate_pl, stats=stats, gamma=sgg, beta=sgbeta, mul=hid_pl)
                x2 = free.pop()
                last = j == d - 1
                plan.conv(ops.conv_params(W[f'{b}.ffn.fc2'], gate_pl, H, Wd, cin_planes=P1, res1=x1, alpha=1.0, out_f32=x2,
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
        norm('norm', cur, out_planes=n_pl)
        resi_conv('conv_after_body', n_pl, first, out_planes=body_pl)  # + conv_first output (arch.py:981, 986)

        y_out = plan.output((n, self.in_chans, H * s, Wd * s), dtype)
        # the last store: x / img_range + mean (arch.py:989)
        reconstruction_head(plan, W, self.upsampler, body_pl, cp, n, H, Wd, s, with_lo, y_out, 1.0 / self.img_range, mean, (x_shape, dtype))
        return set_input
