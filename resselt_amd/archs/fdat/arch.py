"""FDAT ("Fast DAT") on the MI355X engine -- drop-in for ``resselt/archs/fdat/arch.py:632-735`` in eval mode.

Tokens are pixels.  The residual stream is an f32 map and every Linear layer is a k1 launch of the convolution kernels.  Each residual
group runs ``depth_per_group`` pairs of blocks [spatial, channel]:

  block    n1 = LN(x) -> attention -> proj (a)  |  c = GELU(dwconv3x3(n1))  ->  x += AIM(a, c)  ->  x += fc2(smix(GELU(fc1(LN(x)))))
  spatial  square-window attention on DAT's rsa_rect_attention (zero padding to multiples of ws AFTER n1, so padded tokens have
           q = k = v = 0 and are not masked: their logit is the learned bias alone; never shifted); the dense [heads, ws^2, ws^2] bias;
           AIM: f = a * cm + c with cm = sigmoid(W2 GELU(W1 mean_pixels(c))) (DAT's rsa_channel_gate, zero biases)
  channel  DAT's channel attention (rsa_channel_attention_weights -> attn @ v as one k1 launch per image) -> proj;
           AIM: f = a + c * sigmoid(w . a)
  tail     conv3x3 (no bias) + the group input;  trunk: upsampler(conv_after(x_deep) + x_shallow)

rsa_fdat_interact (csrc/fdat.hip) computes the AIM, the residual add and norm2 in one pass; RSA_FDAT_FUSED_INTERACT=0 (read when the model
is built, or the ``fused_interact`` attribute) runs DAT-style separate passes instead: the interaction alone (rsa_fdat_interact writing f),
the residual add (rsa_scale_add) and norm2 (rsa_layernorm).

Front end: with ``unshuffle_mod`` the reflect pad to the unshuffle factor and the PixelUnshuffle are fused into rsa_nchw_to_planes; the output
is cropped to h * scale x w * scale.  Heads (UniUpsampleV3): conv / pixelshuffledirect / pixelshuffle / nearest+conv / dysample are MoSRv2's
(engine/uniupsample.py); transpose+conv runs on rsa_deconv (GELU between the two x4 deconvolutions, cout sliced by 128); pa_up on the
convolutions and rsa_pa_gate; lda on rsa_lda_offsets -> a block-diagonal 3x3 offset convolution -> rsa_lda_attention.
"""

from __future__ import annotations

import math
import os

import torch

from ...engine import cugan as CG
from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ...engine.transformer import HEAD_PAD, LayerPacker, bias_fragments_qk, layernorm, regroup_proj, regroup_qkv
from ...engine.uniupsample import SAMPLE_MODS, SAMPLE_MODS3, Head, OwnMetaUpsample
from ..dat.arch import pad_rows

LDA_RANGE, LDA_EPS = 11.0, 1e-6
MAX_C = 256  # rsa_fdat_interact
RECT_MAX_TOKENS = 256  # rsa_rect_attention


def fused_interact_default() -> bool:
    return os.environ.get('RSA_FDAT_FUSED_INTERACT', '1') != '0'


def v3_layers(upsample: str, scale: int, in_dim: int, out_dim: int, mid_dim: int):
    """UniUpsampleV3's layers with parameters beyond the shared modes: [(kind, index, cout, cin, k)], kind in conv / deconv / pa / lda."""
    if scale == 1 or upsample in SAMPLE_MODS:
        return None
    pow2 = scale & (scale - 1) == 0
    if upsample == 'transpose+conv':
        if scale == 2:
            layers, i = [('deconv', 0, out_dim, in_dim, 4)], 1
        elif scale == 3:
            layers, i = [('deconv', 0, out_dim, in_dim, 3)], 1
        elif scale == 4:
            layers, i = [('deconv', 0, in_dim, in_dim, 4), ('deconv', 2, out_dim, in_dim, 4)], 3
        else:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2, 3, 4')
        return layers + [('conv', i, out_dim, out_dim, 3)]
    if upsample == 'lda':
        layers, i = [], 0
        if mid_dim != in_dim:
            layers, i = [('conv', 0, mid_dim, in_dim, 3)], 2
        return layers + [('lda', i, mid_dim, mid_dim, 0), ('conv', i + 1, out_dim, mid_dim, 3)]
    if upsample == 'pa_up':
        if not pow2 and scale != 3:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
        layers, i, cin = [], 0, in_dim
        for _ in range(int(math.log2(scale)) if pow2 else 1):
            layers += [('conv', i + 1, mid_dim, cin, 3), ('pa', i + 2, mid_dim, mid_dim, 1), ('conv', i + 4, mid_dim, mid_dim, 3)]
            i, cin = i + 6, mid_dim
        return layers + [('conv', i, out_dim, mid_dim, 3)]
    raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')


def fdat_param_shapes(in_ch, dim, num_groups, depth_per_group, heads, ws, hidden, aim_hidden, unshuffle, up: Head, layers):
    """``up``: the head (its MetaUpsample buffer, and the shapes of the shared modes); ``layers``: ``v3_layers`` of the other three, or None."""
    s = ParamShapes()
    buffers: dict = {}
    if unshuffle > 1:
        s.conv('conv_first.1', dim, in_ch * unshuffle * unshuffle, 3)
    else:
        s.conv('conv_first', dim, in_ch, 3)
    for g in range(num_groups):
        for j in range(2 * depth_per_group):
            b = f'groups.{g}.blocks.{j}'
            s.norm(f'{b}.n1', dim)
            s.norm(f'{b}.n2', dim)
            if j % 2 == 0:
                s[f'{b}.attn.bias'] = (heads, ws * ws, ws * ws)
            else:
                s[f'{b}.attn.temp'] = (heads, 1, 1)
            s.linear(f'{b}.attn.qkv', 3 * dim, dim, False)
            s.linear(f'{b}.attn.proj', dim, dim)
            s[f'{b}.conv.0.weight'] = (dim, 1, 3, 3)
            s[f'{b}.inter.sg.0.weight'] = (1, dim, 1, 1)
            s[f'{b}.inter.cg.1.weight'] = (aim_hidden, dim, 1, 1)
            s[f'{b}.inter.cg.3.weight'] = (dim, aim_hidden, 1, 1)
            s.linear(f'{b}.ffn.fc1', hidden, dim, False)
            s.linear(f'{b}.ffn.fc2', dim, hidden, False)
            s[f'{b}.ffn.smix.weight'] = (hidden, 1, 3, 3)
        s[f'groups.{g}.conv.weight'] = (dim, dim, 3, 3)
    s['conv_after.weight'] = (dim, dim, 3, 3)
    up.shapes(s, buffers)
    for kind, i, co, ci, k in layers or []:
        u = f'upsampler.{i}'
        if kind == 'conv':
            s.conv(u, co, ci, k)
        elif kind == 'deconv':
            s[f'{u}.weight'] = (ci, co, k, k)
            s[f'{u}.bias'] = (co,)
        elif kind == 'pa':
            s.conv(f'{u}.conv.0', co, ci, 1)
        else:  # LDA_AQU(mid): reduction 4, one head, k_e = k_u = 3, two groups, rpb
            hid, gc = co // 4, co // 8
            s[f'{u}.relative_position_bias_table'] = (1, 1, 1, 9, hid)
            s[f'{u}.proj_q.weight'] = (hid, co, 1, 1)
            s[f'{u}.proj_k.weight'] = (hid, co, 1, 1)
            s[f'{u}.conv_offset.0.weight'] = (gc, 1, 3, 3)
            s.norm(f'{u}.conv_offset.1', gc)
            s.conv(f'{u}.conv_offset.3', 18, gc, 3)
            s.norm(f'{u}.layer_norm', co)
    return s, buffers


class FDAT(OwnMetaUpsample, EngineModule):  # (the reference's load_state_dict override: arch.py:692-699)
    hyperparameters = {}
    precisions = ('bf16x3', 'bf16')

    def __init__(self, *, num_in_ch: int = 3, num_out_ch: int = 3, scale: int = 4, embed_dim: int = 120, num_groups: int = 4, depth_per_group: int = 3,
                 num_heads: int = 4, window_size: int = 8, ffn_expansion_ratio: float = 2.0, aim_reduction_ratio: int = 8, group_block_pattern=None,
                 drop_path_rate: float = 0.1, mid_dim: int = 64, upsampler_type: str = 'transpose+conv', img_range: float = 1.0,
                 unshuffle_mod: bool = False) -> None:  # fmt: skip
        super().__init__()
        if group_block_pattern not in (None, ['spatial', 'channel'], ('spatial', 'channel')):
            raise NotImplementedError('FDAT engine: the block pattern is [spatial, channel] (what the loader builds)')
        if upsampler_type not in SAMPLE_MODS3:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS3}')
        dim, heads, ws = embed_dim, num_heads, window_size
        if dim > MAX_C:
            raise NotImplementedError(f'FDAT engine: embed_dim {dim} > {MAX_C} (rsa_fdat_interact)')
        if heads < 1 or dim % heads or dim // heads > HEAD_PAD:
            raise NotImplementedError(f'FDAT engine: embed_dim {dim} over {heads} heads: head_dim must divide embed_dim and be <= {HEAD_PAD}')
        if ws < 2 or ws * ws > RECT_MAX_TOKENS:
            raise NotImplementedError(f'FDAT engine: window_size {ws}: window^2 must be in 4..{RECT_MAX_TOKENS} (rsa_rect_attention)')
        aim_hidden = dim // aim_reduction_ratio
        if not 1 <= aim_hidden <= 128:
            raise NotImplementedError(f'FDAT engine: the AIM channel gate width {aim_hidden} must be in 1..128 (rsa_channel_gate)')
        self.unshuffle, self.s_int = 1, scale
        if unshuffle_mod and scale < 3:
            self.unshuffle, self.s_int = 4 // scale, 4
        s_int = self.s_int
        if s_int > 1 and upsampler_type in ('pixelshuffle', 'pa_up', 'lda') and mid_dim % 8:
            raise NotImplementedError(f'FDAT engine: the {upsampler_type} head needs mid_dim a multiple of 8 (got {mid_dim})')
        if s_int > 1 and upsampler_type == 'dysample' and mid_dim != dim and mid_dim % 8:
            raise NotImplementedError(f'FDAT engine: the dysample head needs mid_dim a multiple of 8 (got {mid_dim})')
        if s_int > 1 and upsampler_type == 'lda' and (mid_dim % 16 or mid_dim // 4 > 64):
            raise NotImplementedError(f'FDAT engine: the lda head needs mid_dim a multiple of 16 and at most 256 (rsa_lda_attention; got {mid_dim})')
        if s_int > 1 and upsampler_type == 'transpose+conv' and num_out_ch > 128:
            raise NotImplementedError('FDAT engine: transpose+conv with more than 128 output channels')
        self.in_ch, self.out_ch, self.scale, self.dim, self.num_groups, self.depth = num_in_ch, num_out_ch, scale, dim, num_groups, depth_per_group
        self.heads, self.ws, self.hidden, self.aim_hidden = heads, ws, int(dim * ffn_expansion_ratio), aim_hidden
        self.head, self.mid_dim, self.img_range = upsampler_type, mid_dim, img_range
        self.fused_interact = fused_interact_default()
        self.v3 = v3_layers(upsampler_type, s_int, dim, num_out_ch, mid_dim)
        self.up = Head('upsampler', upsampler_type, s_int, dim, num_out_ch, mid_dim, version=3)  # (no layers of its own where ``v3`` has them)
        shapes, buffers = fdat_param_shapes(num_in_ch, dim, num_groups, depth_per_group, heads, ws, self.hidden, aim_hidden, self.unshuffle, self.up, self.v3)
        build_param_tree(self, shapes, buffers)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        C_, heads, hid = self.dim, self.heads, self.hidden
        cp, P1 = (C_ + 7) // 8, (hid + 7) // 8
        pk = LayerPacker(sd, device, products, lambda name: (int(products), products.fmt))
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln
        zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=device)  # noqa: E731
        conv('conv_first.1' if self.unshuffle > 1 else 'conv_first')
        for g in range(self.num_groups):
            for j in range(2 * self.depth):
                b = f'groups.{g}.blocks.{j}'
                spatial = j % 2 == 0
                ln(f'{b}.n1')
                ln(f'{b}.n2')
                wq, bq = regroup_qkv(sd[f'{b}.attn.qkv.weight'], None, heads, scale_q=spatial)
                lin(f'{b}.attn.qkv', wq, bq)
                lin(f'{b}.attn.proj', regroup_proj(sd[f'{b}.attn.proj.weight'], heads), sd[f'{b}.attn.proj.bias'], cin_planes=heads * HEAD_PAD // 8)
                if spatial:
                    W[f'{b}.attn.bias'] = bias_fragments_qk(sd[f'{b}.attn.bias'])
                    w1 = torch.zeros((self.aim_hidden, cp * 8), dtype=torch.float32, device=device)
                    w1[:, :C_] = sd[f'{b}.inter.cg.1.weight'].reshape(self.aim_hidden, C_)
                    W[f'{b}.inter.cg'] = (w1, zeros(self.aim_hidden), pad_rows(sd[f'{b}.inter.cg.3.weight'].reshape(C_, self.aim_hidden), cp * 8),
                                          zeros(cp * 8))  # fmt: skip
                else:
                    W[f'{b}.attn.temp'] = sd[f'{b}.attn.temp'].reshape(-1).contiguous()
                    W[f'{b}.inter.sg'] = sd[f'{b}.inter.sg.0.weight'].reshape(-1).contiguous()
                W[f'{b}.conv'] = (pad_rows(sd[f'{b}.conv.0.weight'].reshape(C_, 9), cp * 8), zeros(cp * 8))
                lin(f'{b}.ffn.fc1')
                lin(f'{b}.ffn.fc2')
                W[f'{b}.ffn.smix'] = (pad_rows(sd[f'{b}.ffn.smix.weight'].reshape(hid, 9), P1 * 8), zeros(P1 * 8))
            conv(f'groups.{g}.conv')
        conv('conv_after')
        if self.v3 is None:
            self.up.pack(W, sd, products, device)
        else:
            self._pack_v3(W, sd, products, device)
        return W

    def _pack_v3(self, W, sd, products, device):
        cw = lambda w, b, prod=products: ops.ConvWeights.from_oihw(w, b, prod, device=device)  # noqa: E731
        for kind, i, co, ci, k in self.v3:
            u = f'upsampler.{i}'
            if kind == 'conv':
                W[u] = cw(sd[f'{u}.weight'], sd[f'{u}.bias'])
            elif kind == 'pa':
                W[u] = cw(sd[f'{u}.conv.0.weight'], sd[f'{u}.conv.0.bias'])
            elif kind == 'deconv':  # rsa_deconv runs three bf16 products (the only bf16 form it has); cout sliced by 128
                w, b = sd[f'{u}.weight'], sd[f'{u}.bias']
                W[u] = [CG.ResampleWeights.make(w[:, c0 : c0 + 128], b[c0 : c0 + 128], 2 if k == 4 else 3, 1 if k == 4 else 0, True, 3, PF_BF16, device)
                        for c0 in range(0, co, 128)]  # fmt: skip
            else:
                hid, gc = co // 4, co // 8
                ln_w, ln_b = sd[f'{u}.layer_norm.weight'], sd[f'{u}.layer_norm.bias']
                W[f'{u}.ln'] = (ln_w.contiguous(), ln_b.contiguous())
                hp = (hid + 7) // 8
                wqk = torch.zeros((2 * hp * 8, co, 1, 1), dtype=torch.float32, device=device)
                wqk[:hid] = sd[f'{u}.proj_q.weight']
                wqk[hp * 8 : hp * 8 + hid] = sd[f'{u}.proj_k.weight']
                W[f'{u}.qk'] = cw(wqk, None)
                W[f'{u}.dw'] = (sd[f'{u}.conv_offset.0.weight'].reshape(gc, 9).contiguous(), sd[f'{u}.conv_offset.1.weight'].contiguous(),
                                sd[f'{u}.conv_offset.1.bias'].contiguous())  # fmt: skip
                wo = torch.zeros((36, hid, 3, 3), dtype=torch.float32, device=device)  # block-diagonal: group g's 18 offsets read its gc channels
                for g in range(2):
                    wo[18 * g : 18 * g + 18, g * gc : (g + 1) * gc] = sd[f'{u}.conv_offset.3.weight']
                W[f'{u}.off'] = cw(wo, sd[f'{u}.conv_offset.3.bias'].repeat(2))
                W[f'{u}.rpb'] = sd[f'{u}.relative_position_bias_table'].reshape(9, hid).contiguous()
        if self.head == 'pa_up' and self.s_int == 3:  # the nearest x3 map: an identity 1x1 convolution stored through depth-to-space
            eye = torch.eye(self.dim, dtype=torch.float32, device=device).repeat_interleave(9, 0)
            W['dup9'] = cw(eye[:, :, None, None], None)

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per (trunk) pixel: convolutions, Linear layers, both attention kinds, depthwise convolutions; the head at its
        resolution."""
        C_, hid, ntok, u = self.dim, self.hidden, self.ws * self.ws, self.unshuffle
        blk = 3 * C_ * C_ + C_ * C_ + 9 * C_ + C_ * hid + 9 * hid + hid * C_
        macs = 9 * self.in_ch * u * u * C_ + self.num_groups * (self.depth * (2 * blk + 2 * ntok * C_ + 2 * (C_ // self.heads) * C_) + 9 * C_ * C_)
        macs += 9 * C_ * C_
        return (macs + self._head_macs()) // (u * u)

    def _head_macs(self) -> int:
        """MACs of the head per trunk pixel, every layer counted at the resolution it runs at (area relative to the trunk)."""
        s, C_, mid, out = self.s_int, self.dim, self.mid_dim, self.out_ch
        if self.v3 is None:
            layers = self.up.layers
            if s == 1 or self.head in ('conv', 'pixelshuffledirect'):
                return self.up.macs()
            if self.head == 'dysample':
                d = self.up.dys_dim
                pre = 9 * C_ * mid if self.up.dys_index == 2 else 0
                return pre + 2 * d * 8 * s * s + d * out * s * s  # offset and scope at LR, the end convolution at HR
            if self.head == 'pixelshuffle':
                macs, area = 0, 1
                for _, co, ci, k in layers:
                    macs += co * ci * k * k * area
                    if co == out:
                        break
                    if co != mid:  # a shuffling convolution: the next layer runs r^2 times larger
                        area *= co // mid
                return macs
            # nearest+conv: stage j's convolution runs before its upsampling
            stages = len(layers) - 2
            areas = [1] + [4**j for j in range(1, stages)] if s != 3 else [1]
            return sum(9 * C_ * C_ * a for a in areas) + 9 * C_ * C_ * s * s + 9 * C_ * out * s * s
        macs = 0
        if self.head == 'transpose+conv':
            area = 1
            for kind, _, co, ci, k in self.v3:
                macs += ci * co * k * k * area  # a transposed convolution: ci * co * k^2 per INPUT pixel
                if kind == 'deconv':
                    area *= (2 if k == 4 else 3) ** 2
            return macs
        if self.head == 'pa_up':
            area = 9 if s == 3 else 1
            for st in range(0, len(self.v3) - 1, 3):
                if s != 3:
                    area *= 4
                (_, _, co1, ci1, _), (_, _, cop, cip, _), (_, _, co2, ci2, _) = self.v3[st : st + 3]
                macs += (9 * co1 * ci1 + cop * cip + 9 * co2 * ci2) * area
            return macs + 9 * mid * out * area
        hid = mid // 4  # lda
        pre = 9 * C_ * mid if self.v3[0][0] == 'conv' else 0
        hr = 9 * hid + 9 * 18 * hid + 9 * (hid + mid) + 9 * mid * out  # depthwise, offset convolution, scores + P v, final convolution
        return pre + 2 * mid * hid + hr * s * s

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        u, s, C_, heads, ws = self.unshuffle, self.s_int, self.dim, self.heads, self.ws
        Hp, Wp = h0 + (u - h0 % u) % u, w0 + (u - w0 % u) % u
        if Hp - h0 >= h0 or Wp - w0 >= w0:
            raise RuntimeError('input is too small for reflect padding to the unshuffle factor')
        H, Wd = Hp // u, Wp // u
        with_lo = products == 3
        prod, fmt = int(products), products.fmt
        cp, hp = (C_ + 7) // 8, heads * HEAD_PAD // 8
        P1 = (self.hidden + 7) // 8
        dev = plan.device
        lib = L.load()
        Hw, Ww = H + (ws - H % ws) % ws, Wd + (ws - Wd % ws) % ws
        x_pl = plan.planes(n, (c * u * u + 7) // 8, H, Wd, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl, unshuffle=u)  # check_img_size's reflect pad and the PixelUnshuffle, fused

        first = plan.f32map(n, C_, H, Wd)
        pool = [plan.f32map(n, C_, H, Wd) for _ in range(3)]
        a_pl = plan.planes(n, cp, H, Wd, with_lo)  # n1, then n2
        qkv_pl = plan.planes(n, 3 * hp, H, Wd, with_lo)
        att_pl = plan.planes(n, hp, H, Wd, with_lo)
        prj_pl = plan.planes(n, cp, H, Wd, with_lo)
        cb_pl = plan.planes(n, cp, H, Wd, with_lo)
        hid_pl = plan.planes(n, P1, H, Wd, with_lo)
        mix_pl = plan.planes(n, P1, H, Wd, with_lo)
        body_pl = plan.planes(n, cp, H, Wd, with_lo)
        gate = torch.empty((n, cp * 8), dtype=torch.float32, device=dev)
        ws_gate = torch.empty((max(int(lib.rsa_channel_gate_workspace_bytes(n, H, Wd, cp)), 16) // 4,), dtype=torch.float32, device=dev)
        ws_attn = torch.empty((max(int(lib.rsa_channel_attn_workspace_bytes(n, H, Wd, heads)), 16) // 4,), dtype=torch.float32, device=dev)
        zero_bias = torch.zeros((hp * 8,), dtype=torch.float32, device=dev)
        wdyn = torch.zeros((n, int(lib.rsa_packed_weight_bytes(hp * 8, hp, 1, prod)) // 2), dtype=torch.bfloat16, device=dev)  # off-diagonal blocks stay 0
        plan.keep += [gate, ws_gate, ws_attn, zero_bias, wdyn]
        if not self.fused_interact:
            f_map = plan.f32map(n, C_, H, Wd)
            ones = torch.zeros((4 * ((C_ + 3) // 4),), dtype=torch.float32, device=dev)
            ones[:C_] = 1.0
            plan.keep.append(ones)

        def dwconv(weights, src, planes, out, act):
            dp = L.DwConvParams()
            dp.batch, dp.H, dp.W, dp.planes, dp.act, dp.fmt = n, H, Wd, planes, act, src.fmt
            src.bind(dp, 'in')
            dp.weight, dp.bias = weights[0].data_ptr(), weights[1].data_ptr()
            out.bind(dp, 'out')
            plan.launch('rsa_dwconv3x3', dp)

        def spatial_attention(b):
            ap = L.RectAttnParams()
            ap.batch, ap.H, ap.W, ap.Hp, ap.Wp = n, H, Wd, Hw, Ww
            ap.win_h, ap.win_w, ap.shift_h, ap.shift_w = ws, ws, 0, 0
            ap.heads, ap.head0, ap.heads_total, ap.products, ap.fmt = heads, 0, heads, prod, fmt
            qkv_pl.bind(ap, 'qkv')
            ap.bias_frag = W[f'{b}.attn.bias'].data_ptr()
            att_pl.bind(ap, 'out')
            plan.launch('rsa_rect_attention', ap)

        def channel_attention(b):
            cpar = L.ChannelAttnParams()
            cpar.batch, cpar.H, cpar.W, cpar.heads, cpar.head_dim, cpar.products, cpar.fmt = n, H, Wd, heads, C_ // heads, prod, fmt
            cpar.q_hi, cpar.q_lo = qkv_pl.hi_ptr(0), qkv_pl.lo_ptr(0)
            cpar.k_hi, cpar.k_lo = qkv_pl.hi_ptr(hp), qkv_pl.lo_ptr(hp)
            cpar.plane_stride, cpar.batch_stride = qkv_pl.plane_stride, qkv_pl.batch_stride
            cpar.temperature = W[f'{b}.attn.temp'].data_ptr()
            cpar.workspace, cpar.w_packed = ws_attn.data_ptr(), wdyn.data_ptr()
            plan.launch('rsa_channel_attention_weights', cpar, kernels=2)
            for bi in range(n):  # attn @ v: the weights differ per image
                wts = ops.ConvWeights(wdyn[bi], zero_bias, hp * 8, hp * 8, hp, 1, prod, fmt=fmt)
                src = Planes(qkv_pl.hi[bi : bi + 1], None if qkv_pl.lo is None else qkv_pl.lo[bi : bi + 1])
                dst = Planes(att_pl.hi[bi : bi + 1], None if att_pl.lo is None else att_pl.lo[bi : bi + 1])
                plan.conv(ops.conv_params(wts, src, H, Wd, in_plane0=2 * hp, cin_planes=hp, out=dst))

        def channel_gate(b):
            w1, b1, w2, b2 = W[f'{b}.inter.cg']
            gp = L.ChannelGateParams()
            gp.batch, gp.H, gp.W, gp.planes, gp.hidden, gp.relu, gp.fmt = n, H, Wd, cp, self.aim_hidden, 0, fmt
            cb_pl.bind(gp, 'in')
            gp.w1, gp.b1, gp.w2, gp.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
            gp.workspace, gp.gate = ws_gate.data_ptr(), gate.data_ptr()
            plan.launch('rsa_channel_gate', gp, kernels=2)

        def interact(b, mode, x, x_out):
            ip = L.FdatInteractParams()
            ip.batch, ip.H, ip.W, ip.C, ip.mode, ip.fmt = n, H, Wd, C_, mode, fmt
            prj_pl.bind(ip, 'a')
            cb_pl.bind(ip, 'c')
            if mode == 0:
                ip.cm = gate.data_ptr()
            else:
                ip.w = W[f'{b}.inter.sg'].data_ptr()
            g2, b2 = W[f'{b}.n2']
            if self.fused_interact:
                ip.x, ip.x_out = x.data_ptr(), x_out.data_ptr()
                ip.gamma, ip.beta, ip.eps = g2.data_ptr(), b2.data_ptr(), 1e-5
                a_pl.bind(ip, 'out')
                plan.launch('rsa_fdat_interact', ip)
                return
            # three passes over the stream, as DAT's separate launches: the interaction alone into an f32 map, the residual add, norm2
            inplace = x_out is x
            f = f_map if inplace else x_out  # (the first block of a group keeps the group input: f goes to x_out, then x_out += x)
            ip.x_out = f.data_ptr()
            plan.launch('rsa_fdat_interact', ip)
            res = f_map if inplace else x
            plan.launch('rsa_scale_add', dict(res=res, gamma=ones, out=x_out, batch=n, H=H, W=Wd, C=C_))
            layernorm(plan, W, f'{b}.n2', n, H, Wd, C_, x_out, out_planes=a_pl)

        plan.conv(ops.conv_params(W['conv_first.1' if u > 1 else 'conv_first'], x_pl, H, Wd, out_f32=first))
        g_in = first
        for g in range(self.num_groups):
            free = [m for m in pool if m is not g_in]
            cur = g_in
            for j in range(2 * self.depth):
                b = f'groups.{g}.blocks.{j}'
                layernorm(plan, W, f'{b}.n1', n, H, Wd, C_, cur, out_planes=a_pl)
                plan.conv(ops.conv_params(W[f'{b}.attn.qkv'], a_pl, H, Wd, cin_planes=cp, out=qkv_pl))
                if j % 2 == 0:
                    spatial_attention(b)
                else:
                    channel_attention(b)
                plan.conv(ops.conv_params(W[f'{b}.attn.proj'], att_pl, H, Wd, cin_planes=hp, out=prj_pl))
                dwconv(W[f'{b}.conv'], a_pl, cp, cb_pl, L.ACT_GELU)
                xo = free.pop() if cur is g_in else cur  # the group input stays intact for the group's residual
                if j % 2 == 0:
                    channel_gate(b)
                interact(b, j % 2, cur, xo)
                cur = xo
                plan.conv(ops.conv_params(W[f'{b}.ffn.fc1'], a_pl, H, Wd, cin_planes=cp, act=L.ACT_GELU, out=hid_pl))
                dwconv(W[f'{b}.ffn.smix'], hid_pl, P1, mix_pl, L.ACT_NONE)
                nxt = free.pop()
                last = j == 2 * self.depth - 1
                plan.conv(ops.conv_params(W[f'{b}.ffn.fc2'], mix_pl, H, Wd, cin_planes=P1, res1=cur, alpha=1.0, out_f32=nxt, out=body_pl if last else None))
                free.append(cur)
                cur = nxt
            out = free.pop() if g < self.num_groups - 1 else None
            last_group = g == self.num_groups - 1
            plan.conv(ops.conv_params(W[f'groups.{g}.conv'], body_pl, H, Wd, cin_planes=cp, res1=g_in, alpha=1.0, out_f32=out,
                                      out=a_pl if last_group else None))  # fmt: skip
            g_in = out
        # the head's input: conv_after(x_deep) + x_shallow
        f = 1 if self.head == 'conv' else s  # UniUpsampleV3's conv head does not upsample, whatever the scale says
        y = plan.output((n, self.out_ch, H * f, Wd * f), dtype, crop=(h0 * self.scale, w0 * self.scale))
        fe_lo = with_lo or self.head == 'transpose+conv'
        fe = plan.planes(n, cp, H, Wd, fe_lo)
        want32 = (self.v3 is None and self.up.needs_f32_input(W)) or (self.head == 'lda' and s > 1 and self.mid_dim == C_)
        fe32 = plan.f32map(n, C_, H, Wd) if want32 else None
        plan.conv(ops.conv_params(W['conv_after'], a_pl, H, Wd, cin_planes=cp, res1=first, alpha=1.0, out=fe, out_f32=fe32))
        if self.v3 is None:
            self.up.emit(plan, W, fe, fe32, y, with_lo)
        elif self.head == 'transpose+conv':
            self._emit_transpose(plan, W, fe, y, n, H, Wd, with_lo)
        elif self.head == 'pa_up':
            self._emit_pa(plan, W, fe, y, n, H, Wd, with_lo)
        else:
            self._emit_lda(plan, W, fe, fe32, y, n, H, Wd, with_lo)
        return set_input

    def _emit_transpose(self, plan, W, fe, y, n, H, Wd, with_lo):
        t, hh, ww = fe, H, Wd
        for kind, i, co, ci, k in self.v3:
            u = f'upsampler.{i}'
            if kind == 'deconv':
                r = 2 if k == 4 else 3
                o = plan.planes(n, (co + 7) // 8, hh * r, ww * r, True)
                gelu = i == 0 and self.s_int == 4
                for si, wts in enumerate(W[u]):
                    p0 = 16 * si  # 128 channels = 16 planes per slice
                    dst = Planes(o.hi[:, p0:], o.lo[:, p0:])
                    p = CG.resample_params(wts, t, CG.Win(0, 0, hh, ww), out=dst)
                    if gelu:
                        p.act = L.ACT_GELU
                    plan.launch('rsa_deconv', p)
                t, hh, ww = o, hh * r, ww * r
            else:
                plan.conv(ops.conv_params(W[u], t, hh, ww, out_nchw=y))

    def _emit_pa(self, plan, W, fe, y, n, H, Wd, with_lo):
        mid, s = self.mid_dim, self.s_int
        mp = mid // 8
        t, hh, ww = fe, H, Wd
        up2 = s != 3
        if s == 3:
            shuffled = torch.empty((n, self.dim, 3 * H, 3 * Wd), dtype=torch.float32, device=plan.device)
            plan.keep.append(shuffled)
            plan.conv(ops.conv_params(W['dup9'], fe, H, Wd, out_nchw=shuffled, pixel_shuffle=3))
            t = plan.planes(n, (self.dim + 7) // 8, 3 * H, 3 * Wd, with_lo)
            plan.call(lambda src=shuffled, dst=t: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
            hh, ww = 3 * H, 3 * Wd
        layers = self.v3
        for st in range(0, len(layers) - 1, 3):
            (_, i1, _, _, _), (_, i2, _, _, _), (_, i3, _, _, _) = layers[st : st + 3]
            if up2:
                hh, ww = hh * 2, ww * 2
            m = plan.planes(n, mp, hh, ww, with_lo)
            lg = plan.planes(n, mp, hh, ww, with_lo)
            o = plan.planes(n, mp, hh, ww, with_lo)
            plan.conv(ops.conv_params(W[f'upsampler.{i1}'], t, hh, ww, upsample2x=up2, out=m))
            plan.conv(ops.conv_params(W[f'upsampler.{i2}'], m, hh, ww, out=lg))
            self._pa_gate(plan, m, lg, n, hh, ww, mp)
            plan.conv(ops.conv_params(W[f'upsampler.{i3}'], m, hh, ww, act=L.ACT_LRELU, act_param=0.2, out=o))
            t = o
        plan.conv(ops.conv_params(W[f'upsampler.{layers[-1][1]}'], t, hh, ww, out_nchw=y))

    @staticmethod
    def _pa_gate(plan, x, logit, n, h, w, planes):
        plan.launch('rsa_pa_gate', dict(x_hi=x.hi_ptr(), x_lo=x.lo_ptr(), logit_hi=logit.hi_ptr(), logit_lo=logit.lo_ptr(), plane_stride=x.plane_stride,
                                        batch_stride=x.batch_stride, batch=n, H=h, W=w, planes=planes, slope=0.2, fmt=x.fmt, out_hi=x.hi_ptr(), out_lo=x.lo_ptr()))  # fmt: skip

    def _emit_lda(self, plan, W, fe, fe32, y, n, H, Wd, with_lo):
        mid, s = self.mid_dim, self.s_int
        hid = mid // 4
        hp = (hid + 7) // 8
        Ho, Wo = H * s, Wd * s
        layers = self.v3
        if layers[0][0] == 'conv':  # conv in -> mid + LeakyReLU(0.01)
            xl = plan.planes(n, mid // 8, H, Wd, with_lo)
            xl32 = plan.f32map(n, mid, H, Wd)
            plan.conv(ops.conv_params(W['upsampler.0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.01, out=xl, out_f32=xl32))
        else:
            xl, xl32 = fe, fe32
        u = f'upsampler.{layers[-2][1]}'
        nrm = plan.planes(n, mid // 8, H, Wd, with_lo)
        g, be = W[f'{u}.ln']
        lp = L.LayerNormParams()
        lp.batch, lp.H, lp.W, lp.C, lp.eps = n, H, Wd, mid, LDA_EPS
        lp.x_f32, lp.gamma, lp.beta = xl32.data_ptr(), g.data_ptr(), be.data_ptr()
        nrm.bind(lp, 'out')
        lp.out_fmt = nrm.fmt
        plan.launch('rsa_layernorm', lp)
        qk = plan.planes(n, 2 * hp, H, Wd, with_lo)
        plan.conv(ops.conv_params(W[f'{u}.qk'], nrm, H, Wd, out=qk))
        offp = plan.planes(n, hp, Ho, Wo, with_lo)
        dw, lg, lb = W[f'{u}.dw']
        op = L.LdaOffsetsParams()
        op.batch, op.H, op.W, op.Hout, op.Wout, op.hidden, op.groups, op.fmt = n, H, Wd, Ho, Wo, hid, 2, qk.fmt
        qk.bind(op, 'q')
        op.dw_weight, op.gamma, op.beta, op.eps = dw.data_ptr(), lg.data_ptr(), lb.data_ptr(), LDA_EPS
        offp.bind(op, 'out')
        plan.launch('rsa_lda_offsets', op)
        off32 = plan.f32map(n, 36, Ho, Wo)
        plan.conv(ops.conv_params(W[f'{u}.off'], offp, Ho, Wo, out_f32=off32))
        att = plan.planes(n, mid // 8, Ho, Wo, with_lo)
        ap = L.LdaAttnParams()
        ap.batch, ap.H, ap.W, ap.Hout, ap.Wout, ap.hidden, ap.C, ap.groups, ap.fmt = n, H, Wd, Ho, Wo, hid, mid, 2, qk.fmt
        ap.range, ap.scale = LDA_RANGE, hid**-0.5
        qk.bind(ap, 'q')
        qk.bind(ap, 'k', hp)
        xl.bind(ap, 'v')
        ap.offset, ap.rpb = off32.data_ptr(), W[f'{u}.rpb'].data_ptr()
        att.bind(ap, 'out')
        plan.launch('rsa_lda_attention', ap)
        plan.conv(ops.conv_params(W[f'upsampler.{layers[-1][1]}'], att, Ho, Wo, out_nchw=y))
