"""Host-side plumbing shared by the window-attention transformers (SwinIR, HAT, DRCT, DAT, RGT, ATD).

Geometry and weight re-layouts are pure torch (CPU-testable): relative-position indices, shift masks, the head-padded qkv / proj
permutations and the gathers of position-bias tables into the attention kernels' accumulator-fragment order.  The plan helpers emit
the steps these models share: the per-layer weight packer, LayerNorm, the 1conv / 3conv residual tail, the reconstruction heads (each with
its parameter shapes, packing, plan step and MAC count side by side), the two-branch rectangular-window attention, the depthwise 3x3
convolution, the per-pixel statistics and the fused MLP half of csrc/swin_block.hip.
"""

from __future__ import annotations

import ctypes as C
import math

import torch

from . import lib as L
from . import ops

HEAD_PAD = 32  # channels each head occupies in the attention planes


def attn_tiles(ntok: int) -> int:
    """Tiles of 32 tokens the rect-attention kernel is instantiated for."""
    t = (ntok + 31) // 32
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 8


# ---------------------------------------------------------------- geometry (registered buffers of the reference modules)
def relative_position_index(hs: int, ws: int | None = None) -> torch.Tensor:
    """The ``relative_position_index`` buffer of an (hs x ws) window: [hs*ws, hs*ws] rows of a (2hs-1)(2ws-1) bias table
    (SwinIR / DRCT WindowAttention, HAT ``relative_position_index_SA``, DAT Spatial_Attention; ``ws`` defaults to a square window)."""
    ws = hs if ws is None else ws
    coords = torch.stack(torch.meshgrid([torch.arange(hs), torch.arange(ws)], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += hs - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def shift_mask(H: int, W: int, window, shift) -> torch.Tensor:
    """The additive mask [nW, N, N] of shifted (hs x ws) windows over an H x W image shifted by (sh, sw): -100 between tokens of
    different regions.  Kept for state_dict parity only; the kernels derive the mask from the geometry."""
    hs, ws = window
    sh, sw = shift
    img = torch.zeros(H, W)
    cnt = 0
    for a in (slice(0, -hs), slice(-hs, -sh), slice(-sh, None)):
        for b in (slice(0, -ws), slice(-ws, -sw), slice(-sw, None)):
            img[a, b] = cnt
            cnt += 1
    mw = img.view(H // hs, hs, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, hs * ws)
    d = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


# ---------------------------------------------------------------- weight re-layouts
def regroup_qkv(w: torch.Tensor, b: torch.Tensor | None, heads: int, pad: int = HEAD_PAD, scale_q: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """[3C, C] -> [3*heads*pad, C]: row (which, head, d) <- which*C + head*hd + d, zero rows for d >= hd; q rows scaled by hd^-0.5."""
    c3, c = w.shape
    hd = c // heads
    wn = torch.zeros((3, heads, pad, c), dtype=torch.float32, device=w.device)
    bn = torch.zeros((3, heads, pad), dtype=torch.float32, device=w.device)
    wn[:, :, :hd] = w.to(torch.float32).reshape(3, heads, hd, c)
    if b is not None:
        bn[:, :, :hd] = b.to(torch.float32).reshape(3, heads, hd)
    if scale_q:
        scale = hd**-0.5
        wn[0] *= scale
        bn[0] *= scale
    return wn.reshape(3 * heads * pad, c), bn.reshape(-1)


def regroup_proj(w: torch.Tensor, heads: int, pad: int = HEAD_PAD) -> torch.Tensor:
    """[C, C] -> [C, heads*pad]: column (head, d) <- head*hd + d."""
    c = w.shape[0]
    hd = w.shape[1] // heads
    wn = torch.zeros((c, heads, pad), dtype=torch.float32, device=w.device)
    wn[:, :, :hd] = w.to(torch.float32).reshape(c, heads, hd)
    return wn.reshape(c, heads * pad)


def pad_heads(t: torch.Tensor, heads: int, dim: int = 0) -> torch.Tensor:
    """Scatter a length-C axis (head-major, C = heads*hd) into the head-padded layout of length heads*32 (zeros in the pads)."""
    c = t.shape[dim]
    hd = c // heads
    shape = list(t.shape)
    t = t.to(torch.float32).reshape(shape[:dim] + [heads, hd] + shape[dim + 1 :])
    out_shape = shape[:dim] + [heads, HEAD_PAD] + shape[dim + 1 :]
    out = torch.zeros(out_shape, dtype=torch.float32, device=t.device)
    out.narrow(dim + 1, 0, hd).copy_(t)
    return out.reshape(shape[:dim] + [heads * HEAD_PAD] + shape[dim + 1 :]).contiguous()


def bias_fragments_qk(dense: torch.Tensor, qt: int | None = None, kt: int | None = None) -> torch.Tensor:
    """[heads, Nq, Nk] (query, key) position bias -> [heads][qt][kt][lane 64][16] f32 in the S^T accumulator order of rsa_rect_attention:
    lane l, element r  <->  query 32*q + (l & 31),  key 32*k + (r & 3) + 8*(r >> 2) + 4*(l >> 5).  Padded keys get -1e30.
    ``qt`` / ``kt`` default to the tile counts the kernel is instantiated for (``attn_tiles``)."""
    heads, nq, nk = dense.shape
    qt = attn_tiles(nq) if qt is None else qt
    kt = attn_tiles(nk) if kt is None else kt
    full = torch.zeros((heads, 32 * qt, 32 * kt), dtype=torch.float32, device=dense.device)
    full[:, :, nk:] = -1e30
    full[:, :nq, :nk] = dense.to(torch.float32)
    lane = torch.arange(64, device=dense.device)
    r = torch.arange(16, device=dense.device)
    q_in = (lane & 31)[:, None].expand(64, 16)
    k_in = ((r & 3) + 8 * (r >> 2))[None, :] + 4 * (lane >> 5)[:, None]
    out = torch.empty((heads, qt, kt, 64, 16), dtype=torch.float32, device=dense.device)
    for a in range(qt):
        for b in range(kt):
            out[:, a, b] = full[:, 32 * a + q_in, 32 * b + k_in]
    return out.contiguous()


_FRAG_LUT: dict = {}


def _fragment_lut(index: torch.Tensor, window: int, order: str) -> torch.Tensor:
    """Row of the bias table each accumulator element reads (-1: a padded key -> -1e30; -2: a padded query -> 0), in the order of
    `bias_fragments` ('32') or `bias_fragments16` ('16').  It depends on the window and on the index buffer only, which every layer of a
    network shares: built once and reused while the index has the same content (the per-layer gathers were 0.2 s of a SwinIR-L cold
    start: 54 layers x 5 indexing operations)."""
    key = (order, window, str(index.device))
    hit = _FRAG_LUT.get(key)
    if hit is not None and hit[0].shape == index.shape and torch.equal(hit[0], index):
        return hit[1]
    n = window * window
    dev = index.device
    dense = torch.full((64, 64), -2, dtype=torch.long, device=dev)  # [query][key] -> table row
    dense[:, n:] = -1
    dense[:n, :n] = index.reshape(n, n).long()
    lane = torch.arange(64, device=dev)
    if order == '32':  # [qt 2][kt 2][lane 64][16]: query 32*qt + (l & 31), key 32*kt + (r & 3) + 8*(r >> 2) + 4*(l >> 5)
        r = torch.arange(16, device=dev)
        q_in = (lane & 31)[:, None].expand(64, 16)
        k_in = ((r & 3) + 8 * (r >> 2))[None, :] + 4 * (lane >> 5)[:, None]
        lut = torch.stack([torch.stack([dense[32 * qt + q_in, 32 * kt + k_in] for kt in range(2)]) for qt in range(2)])
    else:  # [kt 4][qt 4][lane 64][4]: key 16*kt + 4*(l >> 4) + r, query 16*qt + (l & 15)
        r = torch.arange(4, device=dev)
        q_in = (lane & 15)[:, None].expand(64, 4)
        k_in = 4 * (lane >> 4)[:, None] + r[None, :]
        lut = torch.stack([torch.stack([dense[16 * qt + q_in, 16 * kt + k_in] for qt in range(4)]) for kt in range(4)])
    _FRAG_LUT[key] = (index.clone(), lut)
    return lut


def _gather_fragments(table: torch.Tensor, lut: torch.Tensor, scale: float) -> torch.Tensor:
    t = table.to(torch.float32)
    if scale != 1.0:
        t = t * scale
    g = t[lut.clamp(min=0).reshape(-1)].reshape(*lut.shape, t.shape[1])  # [..., heads]
    pad = torch.where(lut == -1, -1e30, 0.0).to(torch.float32)[..., None]
    return torch.where((lut >= 0)[..., None], g, pad).movedim(-1, 0).contiguous()


def bias_fragments(table: torch.Tensor, index: torch.Tensor, window: int) -> torch.Tensor:
    """table[(2w-1)^2, heads] gathered by index[w^2, w^2] -> [heads][qt 2][kt 2][lane 64][16] f32 in the S^T accumulator order of
    rsa_window_attention (windows of at most 64 tokens): lane l, element r  <->  query 32*qt + (l & 31),
    key 32*kt + (r & 3) + 8*(r >> 2) + 4*(l >> 5).  Padded keys get -1e30."""
    return _gather_fragments(table, _fragment_lut(index, window, '32'), 1.0)


def bias_fragments16(table: torch.Tensor, index: torch.Tensor, window: int) -> torch.Tensor:
    """The same gather in the accumulator order of 16x16 tiles (csrc/swin_block.hip): [heads][kt 4][qt 4][lane 64][4] f32,
    lane l, element r  <->  key 16*kt + 4*(l >> 4) + r,  query 16*qt + (l & 15).  Values are multiplied by log2(e): the kernel's
    softmax runs in base 2 (one v_exp_f32 per logit).  Padded keys get -1e30."""
    return _gather_fragments(table, _fragment_lut(index, window, '16'), math.log2(math.e))


# ---------------------------------------------------------------- pack time
class LayerPacker:
    """Packs the convolution, Linear and LayerNorm layers of a state dict into ``W`` under the module's precision: ``layer_policy(name)``
    gives (products, plane format) of each convolution / Linear layer under 'mixed'; every other mode packs all of them alike."""

    def __init__(self, sd: dict, device, products, layer_policy):
        self.sd, self.device, self.products, self.layer_policy = sd, device, products, layer_policy
        self.W: dict = {}

    def policy(self, name: str) -> tuple[int, int]:
        return self.layer_policy(name) if self.products.name == 'mixed' else (int(self.products), self.products.fmt)

    def conv(self, name: str) -> None:
        prod, fmt = self.policy(name)
        self.W[name] = ops.ConvWeights.from_oihw(self.sd[f'{name}.weight'], self.sd.get(f'{name}.bias'), prod, device=self.device, fmt=fmt)

    def lin(self, name: str, w=None, b=None, cin_planes=None) -> None:
        """An ``nn.Linear`` as a k1 convolution; ``w`` / ``b`` replace the state dict's tensors (re-laid-out weights)."""
        w = self.sd[f'{name}.weight'] if w is None else w
        b = self.sd.get(f'{name}.bias') if b is None else b
        prod, fmt = self.policy(name)
        self.W[name] = ops.ConvWeights.from_oihw(w[:, :, None, None], b, prod, cin_planes=cin_planes, device=self.device, fmt=fmt)

    def ln(self, name: str) -> None:
        self.W[name] = (self.sd[f'{name}.weight'].float().contiguous(), self.sd[f'{name}.bias'].float().contiguous())


# ---------------------------------------------------------------- plan steps
def layernorm(plan, W, name, n, H, Wd, C, x_f32, out_planes=None, out_f32=None) -> None:
    """LayerNorm over the C channels of an f32 token map (``rsa_layernorm``) into split planes and / or an f32 map."""
    g, b = W[name]
    lp = L.LayerNormParams()
    lp.batch, lp.H, lp.W, lp.C, lp.eps = n, H, Wd, C, 1e-5
    lp.x_f32, lp.gamma, lp.beta = x_f32.data_ptr(), g.data_ptr(), b.data_ptr()
    if out_planes is not None:
        out_planes.bind(lp, 'out')
        lp.out_fmt = out_planes.fmt
    lp.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    plan.launch('rsa_layernorm', lp)


def layernorm_on(plan, W, n, H, Wd, C_):
    """``norm(name, x_f32, out_planes=None, out_f32=None)``: ``layernorm`` on one plan's token grid."""
    return lambda name, x_f32, out_planes=None, out_f32=None: layernorm(plan, W, name, n, H, Wd, C_, x_f32, out_planes, out_f32)


# ---------------------------------------------------------------- the 1conv / 3conv tail of a residual group (and conv_after_body)
def tail_layers(name: str, resi: str) -> list[str]:
    """Names of the convolutions of the tail ``name``: one 3x3, or 3x3 (C -> C/4), 1x1, 3x3 (C/4 -> C) with LeakyReLU(0.2) between."""
    return [name] if resi == '1conv' else [f'{name}.0', f'{name}.2', f'{name}.4']


def tail_shapes(s, name: str, C_: int, resi: str) -> None:
    if resi == '1conv':
        s.conv(name, C_, C_, 3)
    else:
        s.conv(f'{name}.0', C_ // 4, C_, 3)
        s.conv(f'{name}.2', C_ // 4, C_ // 4, 1)
        s.conv(f'{name}.4', C_, C_ // 4, 3)


def tail_macs(C_: int, resi: str) -> int:
    return 9 * C_ * C_ if resi == '1conv' else (9 * C_ * (C_ // 4) * 2 + (C_ // 4) ** 2)


class ResidualTail:
    """The plan step of the tail: ``tail(name, src_planes, res, out_f32, out_planes)`` emits the convolutions of ``name`` with the residual
    add that follows them in the last one's epilogue.  A 3conv tail owns the two C/4 scratch planes, allocated once per plan."""

    def __init__(self, plan, W, resi, n, H, Wd, C_, with_lo):
        self.plan, self.W, self.resi, self.H, self.Wd, self.cp = plan, W, resi, H, Wd, (C_ + 7) // 8
        self.q4_a = plan.planes(n, (C_ // 4 + 7) // 8, H, Wd, with_lo) if resi == '3conv' else None
        self.q4_b = plan.planes(n, (C_ // 4 + 7) // 8, H, Wd, with_lo) if resi == '3conv' else None

    def squeeze(self, name, src_planes):
        """The first two convolutions of a 3conv tail; returns the planes its last convolution reads."""
        lre = dict(act=L.ACT_LRELU, act_param=0.2)
        self.plan.conv(ops.conv_params(self.W[f'{name}.0'], src_planes, self.H, self.Wd, cin_planes=self.cp, out=self.q4_a, **lre))
        self.plan.conv(ops.conv_params(self.W[f'{name}.2'], self.q4_a, self.H, self.Wd, out=self.q4_b, **lre))
        return self.q4_b

    def __call__(self, name, src_planes, res, out_f32=None, out_planes=None):
        if self.resi == '1conv':
            last, src, kw = name, src_planes, dict(cin_planes=self.cp)
        else:
            last, src, kw = f'{name}.4', self.squeeze(name, src_planes), {}
        self.plan.conv(ops.conv_params(self.W[last], src, self.H, self.Wd, res1=res, alpha=1.0, out_f32=out_f32, out=out_planes, **kw))


# ---------------------------------------------------------------- reconstruction heads
# 'pixelshuffle'        conv_before_upsample + LeakyReLU -> [conv + PixelShuffle] per factor 2 (or one for 3) -> conv_last
# 'nearest+conv'        conv_before_upsample + LeakyReLU -> [nearest 2x + conv_up + LeakyReLU(0.2)] per factor 2 -> conv_hr -> conv_last
# 'pixelshuffledirect'  one convolution (upsample.0) whose store shuffles
# anything else         conv_last on the body's width, added to the caller's own input (denoising / artefact removal)
HEAD_LAYERS = ('conv_before_upsample.0', 'conv_up1', 'conv_up2', 'conv_up3', 'conv_hr', 'conv_last', 'upsample.0', 'upsample.2', 'upsample.4')


def head_shapes(s, upsampler: str, C_: int, nf: int, out_ch: int, upscale: int) -> None:
    if upsampler == 'pixelshuffle':
        s.pixelshuffle_head(C_, nf, out_ch, upscale)
    elif upsampler == 'nearest+conv':
        s.conv('conv_before_upsample.0', nf, C_, 3)
        for u in range(1, int(math.log2(upscale)) + 1):
            s.conv(f'conv_up{u}', nf, nf, 3)
        s.conv('conv_hr', nf, nf, 3)
        s.conv('conv_last', out_ch, nf, 3)
    elif upsampler == 'pixelshuffledirect':
        s.conv('upsample.0', upscale * upscale * out_ch, C_, 3)
    else:
        s.conv('conv_last', out_ch, C_, 3)


def pack_head(pk: 'LayerPacker') -> None:
    """Pack whichever head layers the state dict holds."""
    for name in HEAD_LAYERS:
        if f'{name}.weight' in pk.sd:
            pk.conv(name)


def pixelshuffle_macs(C_: int, nf: int, out_ch: int, scale: int) -> int:
    """MACs per input pixel of the pixel-shuffle head, each convolution at its own resolution."""
    macs = 9 * C_ * nf
    res = 1
    if scale == 3:
        macs += 9 * nf * 9 * nf
        res = 9
    else:
        for _ in range(int(math.log2(scale))):
            macs += 9 * nf * 4 * nf * res
            res *= 4
    return macs + 9 * nf * out_ch * res


def head_macs(upsampler: str, C_: int, nf: int, out_ch: int, scale: int) -> int:
    if upsampler == 'pixelshuffle':
        return pixelshuffle_macs(C_, nf, out_ch, scale)
    if upsampler == 'nearest+conv':
        macs = 9 * C_ * nf
        res = 1
        for _ in range(int(math.log2(scale))):
            res *= 4
            macs += 9 * nf * nf * res
        return macs + (9 * nf * nf + 9 * nf * out_ch) * res
    return 9 * C_ * scale * scale * out_ch  # one convolution: upsample.0, or conv_last at scale 1


def pixelshuffle_buffers(plan, W, n, H, Wd, nf, with_lo) -> tuple:
    """Buffers of the pixel-shuffle head (conv_before_upsample -> [conv + PixelShuffle] x stages): conv_before_upsample's output planes,
    then per stage the plain tensor the shuffling store writes and its re-layout as planes for the next convolution."""
    y0 = plan.planes(n, nf // 8, H, Wd, with_lo)
    stages = []
    hh, ww, i = H, Wd, 0
    while f'upsample.{i}' in W:
        r = math.isqrt(W[f'upsample.{i}'].cout // nf)
        shuffled = torch.empty((n, nf, hh * r, ww * r), dtype=torch.float32, device=plan.device)
        plan.keep.append(shuffled)
        hh, ww = hh * r, ww * r
        stages.append((f'upsample.{i}', r, shuffled, plan.planes(n, nf // 8, hh, ww, with_lo)))
        i += 2
    return y0, stages


def pixelshuffle_head(plan, W, buffers, src, cin_planes, H, Wd, y_out=None, **final) -> tuple:
    """Emit the head from ``buffers`` (``pixelshuffle_buffers``): returns (planes, h, w) that conv_last reads, and emits conv_last into
    ``y_out`` with the ``final`` store arguments when ``y_out`` is given."""
    y, stages = buffers
    plan.conv(ops.conv_params(W['conv_before_upsample.0'], src, H, Wd, cin_planes=cin_planes, act=L.ACT_LRELU, act_param=0.01, out=y))
    hh, ww = H, Wd
    for name, r, shuffled, ny in stages:
        plan.conv(ops.conv_params(W[name], y, hh, ww, out_nchw=shuffled, pixel_shuffle=r))
        hh, ww = hh * r, ww * r
        plan.call(lambda src=shuffled, dst=ny: ops.nchw_to_planes(src, dst))
        plan.count_launches(1)
        y = ny
    if y_out is not None:
        plan.conv(ops.conv_params(W['conv_last'], y, hh, ww, out_nchw=y_out, **final))
    return y, hh, ww


def reconstruction_head(plan, W, upsampler, src, cin_planes, n, H, Wd, scale, with_lo, y_out, out_scale, out_shift, x_sig, nf=64) -> None:
    """Emit the head ``upsampler`` from the planes ``src`` into ``y_out``; the last store computes ``y * out_scale + out_shift``, or, for the
    bare conv_last, ``y * out_scale`` plus the caller's own input ``x_sig`` = (shape, dtype): (x_norm + y) / range + mean == x + y / range."""
    final = dict(out_scale=out_scale, out_shift=out_shift)
    lre = dict(act=L.ACT_LRELU, act_param=0.2)
    if upsampler == 'pixelshuffle':
        pixelshuffle_head(plan, W, pixelshuffle_buffers(plan, W, n, H, Wd, nf, with_lo), src, cin_planes, H, Wd, y_out, **final)
    elif upsampler == 'nearest+conv':
        y = plan.planes(n, nf // 8, H, Wd, with_lo)
        plan.conv(ops.conv_params(W['conv_before_upsample.0'], src, H, Wd, cin_planes=cin_planes, act=L.ACT_LRELU, act_param=0.01, out=y))
        hh, ww = H, Wd
        for u in range(1, int(math.log2(scale)) + 1):
            hh, ww = hh * 2, ww * 2
            ny = plan.planes(n, nf // 8, hh, ww, with_lo)
            plan.conv(ops.conv_params(W[f'conv_up{u}'], y, hh, ww, upsample2x=True, out=ny, **lre))
            y = ny
        hr = plan.planes(n, nf // 8, hh, ww, with_lo)
        plan.conv(ops.conv_params(W['conv_hr'], y, hh, ww, out=hr, **lre))
        plan.conv(ops.conv_params(W['conv_last'], hr, hh, ww, out_nchw=y_out, **final))
    elif upsampler == 'pixelshuffledirect':
        plan.conv(ops.conv_params(W['upsample.0'], src, H, Wd, cin_planes=cin_planes, out_nchw=y_out, pixel_shuffle=scale, **final))
    else:
        plan.conv(ops.conv_params(W['conv_last'], src, H, Wd, cin_planes=cin_planes, out_nchw=y_out, out_scale=out_scale,
                                  out_base=plan.input_ref(*x_sig), out_base_div=1))  # fmt: skip


# ---------------------------------------------------------------- steps of the rectangular-window models (DAT, RGT)
def branch_geometry(pair, idx: int):
    """(h, w) of a per-branch quantity: branch 1 swaps the rectangle (DAT arch.py:186-191)."""
    return (pair[0], pair[1]) if idx == 0 else (pair[1], pair[0])


def rect_attention(plan, qkv_pl, out_pl, bias_frags, n, H, Wd, split, heads, shifted, products, fmt) -> None:
    """The two branches of a rectangular-window attention (``split`` and its transpose on the two halves of the heads, shifted by half a
    window where ``shifted``): one ``rsa_rect_attention`` launch each.  ``bias_frags`` = the two branches' position-bias fragments."""
    m = max(split)
    for idx in (0, 1):
        ap = L.RectAttnParams()
        ap.batch, ap.H, ap.W, ap.Hp, ap.Wp = n, H, Wd, H + (m - H % m) % m, Wd + (m - Wd % m) % m
        ap.win_h, ap.win_w = branch_geometry(split, idx)
        ap.shift_h, ap.shift_w = branch_geometry([split[0] // 2, split[1] // 2], idx) if shifted else (0, 0)
        ap.heads, ap.head0, ap.heads_total, ap.products = heads // 2, idx * (heads // 2), heads, products
        ap.fmt = fmt
        qkv_pl.bind(ap, 'qkv')
        ap.bias_frag = bias_frags[idx].data_ptr()
        out_pl.bind(ap, 'out')
        plan.launch('rsa_rect_attention', ap)


def dwconv3x3(plan, weights, src, src_plane0, planes, out, out_plane0=0, act=L.ACT_NONE, stats=None, gamma=None, beta=None, mul=None) -> None:
    """``rsa_dwconv3x3`` over ``planes`` planes of ``src`` from ``src_plane0`` into ``out`` from ``out_plane0``; ``weights`` = (weight, bias).
    With ``stats`` / ``gamma`` / ``beta`` the input is layer-normalised per pixel first; with ``mul`` the result is multiplied by those planes.
    (Source, multiplier and output planes of a call share their format.)"""
    dp = L.DwConvParams()
    dp.batch, dp.H, dp.W, dp.planes, dp.act = src.n, src.h, src.w, planes, act
    dp.fmt = src.fmt
    src.bind(dp, 'in', src_plane0)
    dp.weight, dp.bias = weights[0].data_ptr(), weights[1].data_ptr()
    if stats is not None:
        dp.stats, dp.gamma, dp.beta = stats.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    if mul is not None:
        mul.bind(dp, 'mul')
    out.bind(dp, 'out', out_plane0)
    plan.launch('rsa_dwconv3x3', dp)


def plane_stats(plan, src, plane0, channels, stats) -> None:
    """Per-pixel LayerNorm statistics (eps 1e-5) of ``channels`` channels of ``src`` from ``plane0`` into ``stats`` [N, H*W, 2]."""
    plan.launch('rsa_plane_stats_fmt', dict(in_hi=src.hi_ptr(plane0), in_lo=src.lo_ptr(plane0), plane_stride=src.plane_stride, batch_stride=src.batch_stride,
                                            batch=src.n, H=src.h, W=src.w, C=channels, eps=1e-5, fmt=src.fmt, stats=stats))  # fmt: skip


MLP_MAX_C, MLP_MAX_HIDDEN = 256, 512  # limits of rsa_swin_mlp_block (include/resselt_amd.h)


def mlp_block_fits(channels: int, hidden: int) -> bool:
    return channels <= MLP_MAX_C and channels % 4 == 0 and hidden <= MLP_MAX_HIDDEN


def mlp_block(plan, norm, fc1, fc2, n, h, w, channels, hidden, products, x_f32, out_f32, out_planes=None, eps=1e-5):
    """``out = x + fc2(GELU(fc1(LayerNorm(x))))`` in one launch (reference archs/swinir/arch.py:331-335 with Mlp.forward :34-40; the
    same lines close a HAT block, archs/hat/arch.py).  ``norm`` = (gamma, beta) f32 tensors, ``fc1`` / ``fc2`` = ops.ConvWeights of the
    Linear layers, ``x_f32`` / ``out_f32`` = f32 NCHW4c maps (may be the same), ``out_planes`` = optional split-plane copy."""
    g, be = norm
    mp = L.SwinMlpBlockParams()
    if fc1.products != fc2.products or fc1.fmt != fc2.fmt:
        raise ValueError('fc1 and fc2 must be packed for the same arithmetic')
    # (the arithmetic is what the weights were packed for: an architecture's per-layer policy may run this half in one fp16 product)
    mp.batch, mp.H, mp.W, mp.C, mp.hidden, mp.products, mp.eps = n, h, w, channels, hidden, fc1.products, eps
    mp.fmt = fc1.fmt
    mp.x, mp.gamma, mp.beta = x_f32.data_ptr(), g.data_ptr(), be.data_ptr()
    mp.w1, mp.b1 = fc1.packed_for(0).data_ptr(), fc1.bias.data_ptr()
    mp.w2, mp.b2 = fc2.packed_for(0).data_ptr(), fc2.bias.data_ptr()
    mp.out = out_f32.data_ptr()
    if out_planes is not None:
        out_planes.bind(mp, 'out')
    plan.launch('rsa_swin_mlp_block', mp)
