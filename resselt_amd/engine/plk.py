"""PLKSR building blocks: packing of the large-kernel weights, the pack-time folds of the sparse large-kernel variants, and descriptor
builders for ``rsa_plk_conv`` / ``rsa_group_norm_*`` / ``rsa_ea_gate`` (csrc/plksr.hip).  The folds and the packing run once at load time;
nothing here runs in ``forward``."""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import lib as L
from .tensors import PF_F16, Planes

GN_EPS = 1e-5  # nn.GroupNorm default (rplksr.py:94)


# ------------------------------------------------------------------------------------------------------------------ pack-time folds
def fold_rect_sparse(mn_w, mn_b, nm_w, nm_b, nn_w, nn_b, k: int):
    """RectSparsePLKConv2d (plksr.py:96-118): m x n + n x m + n x n convolutions, all zero-padded 'same', as ONE k x k kernel and bias."""

    def pad_to(w):
        kh, kw = w.shape[2], w.shape[3]
        return F.pad(w, ((k - kw) // 2, (k - kw) // 2, (k - kh) // 2, (k - kh) // 2))

    return pad_to(mn_w) + pad_to(nm_w) + pad_to(nn_w), mn_b + nm_b + nn_b


def fold_sparse(convs, k: int):
    """SparsePLKConv2d (plksr.py:121-240): a list of (weight, bias, dilation) convolutions, each zero-padded 'same', as ONE k x k kernel
    and bias (the dilated taps placed on the k x k grid; the reference's own ``convert``)."""
    w_sum, b_sum = 0.0, 0.0
    for w, b, d in convs:
        ks = w.shape[2]
        rep = (ks - 1) * d + 1
        if rep > k:
            raise NotImplementedError(f'SparsePLK: a {ks}x{ks} kernel at dilation {d} spans {rep} > kernel_size {k}')
        dense = w.new_zeros(w.shape[0], w.shape[1], rep, rep)
        dense[:, :, ::d, ::d] = w
        off = (k - rep) // 2
        w_sum = w_sum + F.pad(dense, (off, off, off, off))
        b_sum = b_sum + b
    return w_sum, b_sum


# ------------------------------------------------------------------------------------------------------------------ rsa_plk_conv
def pack_plk_weights(w: torch.Tensor, products: int, fmt: int) -> torch.Tensor:
    """OIHW [pdim][pdim][K][K] -> the A-fragment blob of rsa_plk_conv (include/resselt_amd.h), a 16-bit container tensor."""
    pdim, cin, k, k2 = w.shape
    if pdim != cin or k != k2 or pdim % 8:
        raise ValueError(f'PLK weights must be [pdim, pdim, K, K] with pdim a multiple of 8, got {tuple(w.shape)}')
    P, S, CT = pdim // 8, (k * k + 3) // 4, (pdim // 8 + 1) // 2
    wt = torch.zeros((CT * 16, pdim, S * 4), dtype=torch.float32, device=w.device)
    wt[:pdim, :, : k * k] = w.to(torch.float32).reshape(pdim, pdim, k * k)
    # [ct][cout16][p][j][s][grp] -> [p][s][ct][grp][cout16][j]: lane = 16 grp + cout16
    wt = wt.reshape(CT, 16, P, 8, S, 4).permute(2, 4, 0, 5, 1, 3).reshape(P, S, CT, 1, 64, 8)
    dt = torch.float16 if fmt == PF_F16 else torch.bfloat16
    hi = wt.to(dt)
    parts = [hi]
    if products == 3:
        parts.append((wt - hi.to(torch.float32)).to(dt))
    blob = torch.cat(parts, dim=3).contiguous().view(torch.bfloat16).reshape(-1)
    nbytes = int(L.load().rsa_plk_packed_weight_bytes(k, P, products))
    if blob.numel() * 2 != nbytes:
        raise AssertionError(f'PLK blob is {blob.numel() * 2} bytes, the library expects {nbytes}')
    return blob


def plk_bias(b: torch.Tensor) -> torch.Tensor:
    pdim = b.numel()
    out = torch.zeros(((pdim // 8 + 1) // 2) * 16, dtype=torch.float32, device=b.device)
    out[:pdim] = b.to(torch.float32)
    return out


def plk_params(blob: torch.Tensor, bias: torch.Tensor, k: int, products: int, x: Planes, out: Planes, out_plane_off: int) -> L.PlkConvParams:
    p = L.PlkConvParams()
    p.batch, p.H, p.W, p.ksize, p.products, p.fmt = x.n, x.h, x.w, k, int(products), x.fmt
    p.planes = _planes_of(blob, k, products)
    if p.planes > x.planes or out_plane_off + p.planes > out.planes or (out.n, out.h, out.w) != (x.n, x.h, x.w) or out.fmt != x.fmt:
        raise ValueError('rsa_plk_conv: input / output planes do not match the layer')
    p.in_hi, p.in_lo = x.hi_ptr(), (x.lo_ptr() if int(products) == 3 else None)
    if int(products) == 3 and not x.has_lo(0, p.planes):
        raise ValueError('rsa_plk_conv: three products need lo planes')
    p.in_plane_stride, p.in_batch_stride = x.plane_stride, x.batch_stride
    p.w_packed, p.bias = blob.data_ptr(), bias.data_ptr()
    p.out_hi = out.hi_ptr()
    p.out_lo = out.lo_ptr() if out.has_lo(out_plane_off, p.planes) else None
    p.out_plane_stride, p.out_batch_stride, p.out_plane_off = out.plane_stride, out.batch_stride, out_plane_off
    return p


def _planes_of(blob: torch.Tensor, k: int, products: int) -> int:
    lib = L.load()
    for planes in range(1, 9):
        if int(lib.rsa_plk_packed_weight_bytes(k, planes, int(products))) == blob.numel() * 2:
            return planes
    raise ValueError('PLK blob size matches no plane count')


def plk_conv(p: L.PlkConvParams, stream: int) -> None:
    L.launch('rsa_plk_conv', p, stream)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def group_norm_workspace(n: int, h: int, w: int, groups: int, device) -> torch.Tensor:
    nbytes = int(L.load().rsa_group_norm_workspace_bytes(n, h, w, groups))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def group_norm_stats_args(x_f32: torch.Tensor, C_: int, groups: int, workspace: torch.Tensor, stats: torch.Tensor, eps: float = GN_EPS) -> dict:
    """The keyword arguments of ``rsa_group_norm_stats`` (for ``Plan.launch`` / ``lib.call``)."""
    n, _, h, w, _ = x_f32.shape
    return dict(x_f32=x_f32, batch=n, H=h, W=w, C=C_, groups=groups, eps=eps, workspace=workspace, stats=stats)


def group_norm_stats(x_f32: torch.Tensor, C_: int, groups: int, workspace: torch.Tensor, stats: torch.Tensor, stream: int, eps: float = GN_EPS) -> None:
    L.call('rsa_group_norm_stats', stream, **group_norm_stats_args(x_f32, C_, groups, workspace, stats, eps))


def group_norm_apply_params(x_f32: torch.Tensor, C_: int, groups: int, stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                            skip_f32: torch.Tensor | None, out: Planes | None, out_f32: torch.Tensor | None) -> L.GroupNormApplyParams:  # fmt: skip
    n, _, h, w, _ = x_f32.shape
    p = L.GroupNormApplyParams()
    p.batch, p.H, p.W, p.C, p.groups = n, h, w, C_, groups
    p.x_f32, p.stats, p.gamma, p.beta = x_f32.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    p.skip_f32 = None if skip_f32 is None else skip_f32.data_ptr()
    if out is not None:
        if (out.n, out.h, out.w) != (n, h, w) or out.planes * 8 < C_:
            raise ValueError('group_norm_apply: output planes do not match')
        p.out_hi, p.out_lo = out.hi_ptr(), (out.lo_ptr() if out.has_lo(0, C_ // 8) else None)
        p.out_plane_stride, p.out_batch_stride, p.out_fmt = out.plane_stride, out.batch_stride, out.fmt
    p.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    return p


def group_norm_apply(p: L.GroupNormApplyParams, stream: int) -> None:
    L.launch('rsa_group_norm_apply', p, stream)


# ------------------------------------------------------------------------------------------------------------------ EA gate
def ea_gate_params(g_f32: torch.Tensor, x: Planes, out: Planes, C_: int) -> L.EaGateParams:
    p = L.EaGateParams()
    p.batch, p.H, p.W, p.C = x.n, x.h, x.w, C_
    if tuple(g_f32.shape) != (x.n, C_ // 4, x.h, x.w, 4) or (out.n, out.h, out.w) != (x.n, x.h, x.w) or out.fmt != x.fmt:
        raise ValueError('ea_gate: operands do not match')
    p.g_f32 = g_f32.data_ptr()
    p.x_hi, p.x_lo = x.hi_ptr(), (x.lo_ptr() if x.has_lo(0, C_ // 8) else None)
    p.x_plane_stride, p.x_batch_stride = x.plane_stride, x.batch_stride
    p.out_hi, p.out_lo = out.hi_ptr(), (out.lo_ptr() if out.has_lo(0, C_ // 8) else None)
    p.out_plane_stride, p.out_batch_stride, p.fmt = out.plane_stride, out.batch_stride, x.fmt
    return p


def ea_gate(p: L.EaGateParams, stream: int) -> None:
    L.launch('rsa_ea_gate', p, stream)
