"""Host side of the Real-CUGAN kernels (csrc/cugan.hip): weight packing of the phase GEMMs and descriptor builders.

A ``Win`` is a window of a grid (origin + size in pixels): include/resselt_amd.h, "Real-CUGAN ops".
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from . import lib as L
from .ops import current_stream_ptr, pad_bias, rsa_dtype
from .pack import split_halves
from .tensors import _PF_DTYPE, PF_BF16, PF_F16, Planes


@dataclass(frozen=True)
class Win:
    y0: int
    x0: int
    h: int
    w: int

    def shrink(self, k: int) -> 'Win':
        return Win(self.y0 + k, self.x0 + k, self.h - 2 * k, self.w - 2 * k)


def _ct_store(cout: int) -> int:
    """cout tiles of a packed blob: the kernel's instantiation (1, 2, 4 or 8 tiles of 16 channels)."""
    ct = (cout + 15) // 16
    return 1 if ct <= 1 else 2 if ct <= 2 else 4 if ct <= 4 else 8


def phase_taps(ksize: int, stride: int, transposed: bool) -> list[tuple[int, int]]:
    """(phase index r, taps per axis) -- rsa_deconv's phase r uses weight taps stride * d + r, d < ceil((k - r) / stride)."""
    if not transposed:
        return [(0, ksize)]
    return [(r, (ksize - r + stride - 1) // stride) for r in range(stride)]


def deconv_out(n: int, ksize: int, stride: int, pad: int) -> int:
    return (n - 1) * stride - 2 * pad + ksize


def pack_resample_weights(w: torch.Tensor, stride: int, transposed: bool, products: int, fmt: int = PF_BF16) -> torch.Tensor:
    """Weights -> the A-fragment blob of rsa_deconv / rsa_conv_s2: [phase][K step][cout tile][hi|lo][lane 64][8].

    ``w`` is [cin][cout][k][k] (nn.ConvTranspose2d) when ``transposed``, else [cout][cin][k][k] (nn.Conv2d).  Lane l of step s holds
    A[16 ct + (l & 15)][unit 4 s + (l >> 4)][0..7], a unit being (tap, input plane of 8 channels) in tap-major order, the taps of a phase
    row-major; phases row-major over (r_y, r_x); zero past the phase's taps, past cin and past cout."""
    w = w.detach().to(torch.float32)
    wt = w.permute(1, 0, 2, 3) if transposed else w  # [cout][cin][k][k]
    cout, cin, k, _ = wt.shape
    cp = (cin + 7) // 8
    axes = phase_taps(k, stride, transposed)
    tmax = max(t for _, t in axes)
    smax = (tmax * tmax * cp + 3) // 4
    cts = _ct_store(cout)
    nph = len(axes) ** 2
    A = torch.zeros((nph, 16 * cts, 4 * smax, 8), dtype=torch.float32, device=w.device)
    for py, (ry, ty) in enumerate(axes):
        for px, (rx, tx) in enumerate(axes):
            ph = py * len(axes) + px
            for dy in range(ty):
                for dx in range(tx):
                    ky, kx = (stride * dy + ry, stride * dx + rx) if transposed else (dy, dx)
                    t = dy * tx + dx
                    blk = torch.zeros((cout, cp * 8), dtype=torch.float32, device=w.device)
                    blk[:, :cin] = wt[:, :, ky, kx]
                    A[ph, :cout, t * cp : (t + 1) * cp, :] = blk.reshape(cout, cp, 8)
    frag = A.reshape(nph, cts, 16, smax, 4, 8).permute(0, 3, 1, 4, 2, 5).reshape(nph, smax, cts, 1, 64, 8)
    hi, lo = split_halves(frag, _PF_DTYPE[fmt])
    blob = torch.cat([hi, lo], 3) if products == 3 else hi
    return blob.contiguous().view(torch.bfloat16).reshape(-1)


def packed_bytes(ksize: int, stride: int, transposed: bool, cin_planes: int, cout: int, products: int) -> int:
    return int(L.load().rsa_resample_packed_weight_bytes(ksize, stride, int(transposed), cin_planes, cout, products))


@dataclass
class ResampleWeights:
    """One rsa_deconv / rsa_conv_s2 layer's device-resident parameters."""

    blob: torch.Tensor
    bias: torch.Tensor  # f32, padded to 16
    raw_absmax: float
    cin: int
    cout: int
    ksize: int
    stride: int
    pad: int
    transposed: bool
    products: int
    fmt: int

    @staticmethod
    def make(w, b, stride: int, pad: int, transposed: bool, products: int, fmt: int, device) -> 'ResampleWeights':
        w = w.detach().to(device=device, dtype=torch.float32)
        cout = w.shape[1] if transposed else w.shape[0]
        cin = w.shape[0] if transposed else w.shape[1]
        blob = pack_resample_weights(w, stride, transposed, int(products), fmt)
        return ResampleWeights(blob, pad_bias(b, cout, device), float(w.abs().max()), cin, cout, w.shape[2], stride, pad, transposed, int(products), fmt)


def _check_window(win: Win, p: Planes, what: str) -> None:
    if win.y0 < 0 or win.x0 < 0 or win.h < 1 or win.w < 1 or win.y0 + win.h > p.h or win.x0 + win.w > p.w:
        raise ValueError(f'{what}: window {win} outside a {p.h}x{p.w} grid')


def resample_params(wts: ResampleWeights, x: Planes, win_in: Win, *, out: Planes | None = None, out_f32: torch.Tensor | None = None,
                    out_y0: int = 0, out_x0: int = 0, res: Planes | None = None, res_y0: int = 0, res_x0: int = 0,
                    lrelu: bool = False) -> L.ResampleConvParams:  # fmt: skip
    """Fill one ``rsa_resample_conv_params`` (rsa_deconv when ``wts.transposed``, else rsa_conv_s2)."""
    _check_window(win_in, x, 'resample input')
    cp = (wts.cin + 7) // 8
    if x.planes < cp or x.fmt != wts.fmt:
        raise ValueError('resample: input planes do not match the packed weights')
    if wts.transposed:
        oh, ow = deconv_out(win_in.h, wts.ksize, wts.stride, wts.pad), deconv_out(win_in.w, wts.ksize, wts.stride, wts.pad)
    else:
        oh, ow = win_in.h // 2, win_in.w // 2
    if out is None and out_f32 is None:
        raise ValueError('resample: no output')
    gh, gw = (out.h, out.w) if out is not None else (out_f32.shape[2], out_f32.shape[3])
    if out_f32 is not None and (tuple(out_f32.shape) != (x.n, (wts.cout + 3) // 4, gh, gw, 4) or not out_f32.is_contiguous()):
        raise ValueError('resample: out_f32 must be a contiguous f32 map of the output grid')
    if out_y0 < 0 or out_x0 < 0 or out_y0 + oh > gh or out_x0 + ow > gw:
        raise ValueError(f'resample: output window ({out_y0}, {out_x0}, {oh}, {ow}) outside a {gh}x{gw} grid')
    p = L.ResampleConvParams()
    p.batch, p.ksize, p.stride, p.pad = x.n, wts.ksize, wts.stride, wts.pad
    p.cin_planes, p.cout, p.products, p.fmt = cp, wts.cout, wts.products, wts.fmt
    p.in_hi = x.hi_ptr()
    p.in_lo = x.lo_ptr() if wts.products == 3 else None
    if wts.products == 3 and not x.has_lo(0, cp):
        raise ValueError('resample: three products need lo planes')
    p.in_plane_stride, p.in_batch_stride = x.plane_stride, x.batch_stride
    p.in_W, p.in_y0, p.in_x0, p.in_h, p.in_w = x.w, win_in.y0, win_in.x0, win_in.h, win_in.w
    p.act, p.act_param = (L.ACT_LRELU, 0.1) if lrelu else (L.ACT_NONE, 0.0)
    p.w_packed, p.bias = wts.blob.data_ptr(), wts.bias.data_ptr()
    if res is not None:
        if res.n != x.n or res.planes < (wts.cout + 7) // 8 or res_y0 + oh > res.h or res_x0 + ow > res.w or res.fmt != wts.fmt:
            raise ValueError('resample: residual window does not match')
        p.res_hi = res.hi_ptr()
        p.res_lo = res.lo_ptr() if res.has_lo(0, (wts.cout + 7) // 8) else None
        p.res_plane_stride, p.res_batch_stride = res.plane_stride, res.batch_stride
        p.res_W, p.res_y0, p.res_x0 = res.w, res_y0, res_x0
    p.out_H, p.out_W, p.out_y0, p.out_x0 = gh, gw, out_y0, out_x0
    if out is not None:
        if out.n != x.n or out.planes < (wts.cout + 7) // 8 or out.fmt != wts.fmt:
            raise ValueError('resample: output planes do not match')
        p.out_hi = out.hi_ptr()
        p.out_lo = out.lo_ptr() if out.has_lo(0, (wts.cout + 7) // 8) else None
        p.out_plane_stride, p.out_batch_stride = out.plane_stride, out.batch_stride
    p.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    return p


def resample_flop_bytes(p: L.ResampleConvParams, transposed: bool) -> tuple[int, int]:
    """Algorithmic work of one launch: 2 * MACs of the reference layer, and the bytes of its operands read / written once (weights excluded)."""
    if transposed:
        oh, ow = deconv_out(p.in_h, p.ksize, p.stride, p.pad), deconv_out(p.in_w, p.ksize, p.stride, p.pad)
        macs = p.batch * p.in_h * p.in_w * p.ksize * p.ksize * p.cin_planes * 8 * p.cout
    else:
        oh, ow = p.in_h // 2, p.in_w // 2
        macs = p.batch * oh * ow * 4 * p.cin_planes * 8 * p.cout
    half = 2 if p.products == 3 else 1
    nbytes = p.batch * p.in_h * p.in_w * p.cin_planes * 16 * half
    oplanes = (p.cout + 7) // 8
    px = p.batch * oh * ow
    if p.out_hi:
        nbytes += px * oplanes * 16 * (2 if p.out_lo else 1)
    if p.res_hi:
        nbytes += px * oplanes * 16 * (2 if p.res_lo else 1)
    if p.out_f32:
        nbytes += px * ((p.cout + 3) // 4) * 16
    return 2 * macs, nbytes


def run_resample(p: L.ResampleConvParams, transposed: bool, stream: int) -> None:
    L.launch('rsa_deconv' if transposed else 'rsa_conv_s2', p, stream)


# ---------------------------------------------------------------------------------------------------------------- region SE
@dataclass
class SEWeights:
    w1: torch.Tensor  # [hidden][C]
    b1: torch.Tensor
    w2: torch.Tensor  # [C][hidden]
    b2: torch.Tensor

    @staticmethod
    def make(w1, b1, w2, b2, device) -> 'SEWeights':
        f = lambda t: t.detach().to(device=device, dtype=torch.float32).reshape(t.shape[0], -1).contiguous()  # noqa: E731
        return SEWeights(f(w1), b1.detach().to(device=device, dtype=torch.float32).contiguous(), f(w2), b2.detach().to(device=device, dtype=torch.float32).contiguous())


def region_se_params(se: SEWeights, x: Planes, win: Win, workspace: torch.Tensor, gate: torch.Tensor) -> L.RegionSEParams:
    _check_window(win, x, 'region_se')
    hidden, C_ = se.w1.shape
    if C_ != 8 * x.planes:
        raise ValueError(f'region_se: {C_} channels against {x.planes} planes')
    need = int(L.load().rsa_region_se_workspace_bytes(x.n, win.h, x.planes))
    if workspace.numel() * workspace.element_size() < need or gate.numel() < x.n * C_:
        raise ValueError('region_se: workspace / gate too small')
    p = L.RegionSEParams()
    p.batch, p.planes, p.hidden, p.fmt = x.n, x.planes, hidden, x.fmt
    x.bind(p, 'x')
    p.W, p.y0, p.x0, p.h, p.w = x.w, win.y0, win.x0, win.h, win.w
    p.w1, p.b1, p.w2, p.b2 = se.w1.data_ptr(), se.b1.data_ptr(), se.w2.data_ptr(), se.b2.data_ptr()
    p.workspace, p.gate = workspace.data_ptr(), gate.data_ptr()
    return p


def region_se_workspace(n: int, h: int, planes: int, device) -> torch.Tensor:
    nbytes = int(L.load().rsa_region_se_workspace_bytes(n, h, planes))
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


# ---------------------------------------------------------------------------------------------------------------- input / output stages
def input_params(x: torch.Tensor, shape, out: Planes, pad_top: int, pad_left: int, unshuffle: int, scale: float, shift: float) -> L.CuganInputParams:
    """``shape`` = (N, C, h, w) of the image (a uint8 image is [N, h, w, C])."""
    n, c, h, w = shape
    p = L.CuganInputParams()
    p.x, p.dtype = x.data_ptr(), rsa_dtype(x.dtype)
    p.batch, p.C, p.h, p.w = n, c, h, w
    p.pad_top, p.pad_left, p.unshuffle = pad_top, pad_left, unshuffle
    p.in_scale, p.in_shift = scale, shift
    p.out_H, p.out_W, p.fmt = out.h, out.w, out.fmt
    p.out_hi = out.hi_ptr()
    p.out_lo = out.lo_ptr() if out.has_lo(0, (c * unshuffle * unshuffle + 7) // 8) else None
    p.out_plane_stride, p.out_batch_stride = out.plane_stride, out.batch_stride
    if out.n != n or out.planes < (c * unshuffle * unshuffle + 7) // 8:
        raise ValueError('cugan_input: output planes do not match')
    return p


def output_params(fmap: torch.Tensor, channels: int, y0: int, x0: int, r: int, out: torch.Tensor, out_hw, base: torch.Tensor | None = None,
                  base_hw=(0, 0), base_div: int = 1, base_scale: float = 1.0, base_shift: float = 0.0, out_shift: float = 0.0,
                  out_div: float = 1.0) -> L.CuganOutputParams:  # fmt: skip
    n, p4, mh, mw, _ = fmap.shape
    if p4 * 4 < channels * r * r or fmap.dtype != torch.float32 or not fmap.is_contiguous():
        raise ValueError('cugan_output: the map does not hold C r^2 channels')
    p = L.CuganOutputParams()
    p.map, p.batch, p.C = fmap.data_ptr(), n, channels
    p.map_H, p.map_W, p.y0, p.x0, p.pixel_shuffle = mh, mw, y0, x0, r
    p.out_h, p.out_w = out_hw
    p.dtype, p.out = rsa_dtype(out.dtype), out.data_ptr()
    if base is not None:
        if base.dtype != out.dtype or not base.is_contiguous():
            raise ValueError('cugan_output: the base image must be a contiguous tensor of the output dtype')
        p.base = base.data_ptr()
        p.base_h, p.base_w = base_hw
        p.base_div = base_div
    p.base_scale, p.base_shift, p.out_shift, p.out_div = base_scale, base_shift, out_shift, out_div
    return p


def run(fn: str, p, stream: int | None = None, device=None) -> None:
    """Launch one ``(params*, stream)`` entry point on ``stream`` (default: the current stream of ``device``)."""
    L.launch(fn, p, current_stream_ptr(device) if stream is None else stream)


__all__ = ['Win', 'PF_BF16', 'PF_F16', 'phase_taps', 'deconv_out', 'pack_resample_weights', 'ResampleWeights', 'resample_params', 'SEWeights',
           'region_se_params', 'region_se_workspace', 'input_params', 'output_params', 'run', 'run_resample', 'resample_flop_bytes']  # fmt: skip
