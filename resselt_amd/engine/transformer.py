"""Host-side plumbing shared by the window-attention transformers (SwinIR, HAT, DRCT, DAT).

Geometry and weight re-layouts are pure torch (CPU-testable): relative-position indices, shift masks, the head-padded qkv / proj
permutations and the gathers of position-bias tables into the attention kernels' accumulator-fragment order.  The plan helpers emit
the steps every one of these models shares: the per-layer weight packer, LayerNorm, the pixel-shuffle reconstruction head and the
fused MLP half of csrc/swin_block.hip.
"""

from __future__ import annotations

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
        lp.out_hi, lp.out_lo = out_planes.hi_ptr(), out_planes.lo_ptr()
        lp.out_plane_stride, lp.out_batch_stride = out_planes.plane_stride, out_planes.batch_stride
        lp.out_fmt = out_planes.fmt
    lp.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    plan.launch('rsa_layernorm', lp)


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


def pixelshuffle_head(plan, W, buffers, src, cin_planes, H, Wd) -> tuple:
    """Emit the head up to conv_last: returns (planes, h, w) that conv_last reads.  ``buffers`` from ``pixelshuffle_buffers``."""
    y, stages = buffers
    plan.conv(ops.conv_params(W['conv_before_upsample.0'], src, H, Wd, cin_planes=cin_planes, act=L.ACT_LRELU, act_param=0.01, out=y))
    hh, ww = H, Wd
    for name, r, shuffled, ny in stages:
        plan.conv(ops.conv_params(W[name], y, hh, ww, out_nchw=shuffled, pixel_shuffle=r))
        hh, ww = hh * r, ww * r
        plan.call(lambda src=shuffled, dst=ny: ops.nchw_to_planes(src, dst))
        plan.count_launches(1)
        y = ny
    return y, hh, ww


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
        mp.out_hi, mp.out_lo = out_planes.hi_ptr(), out_planes.lo_ptr()
        mp.out_plane_stride, mp.out_batch_stride = out_planes.plane_stride, out_planes.batch_stride
    plan.launch('rsa_swin_mlp_block', mp)
