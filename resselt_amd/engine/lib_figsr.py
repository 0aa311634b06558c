"""ctypes mirrors and signature rows of include/resselt_amd_figsr.h (``rsa_figsr_mix``, ``rsa_figsr_band_packed_weight_bytes``,
``rsa_figsr_input``, ``rsa_figsr_output``; csrc/figsr.hip), registered with ``lib.extend``, and the host-side packing of
``rsa_figsr_mix``'s band weights (beside ``engine/plk.py``'s ``pack_plk_weights``, whose lane layout it shares).

Field order and types are the ABI; tests/test_capi_headers.py compares the mirrors and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import lib as L
from .tensors import PF_F16


class FigsrMixParams(C.Structure):
    """Mirror of ``struct rsa_figsr_mix_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'fmt', 'products', 'ksize', 'gc', 'planes', 'pass_planes', 'reserved0') + L._ptr('w_packed', 'bias_w', 'bias_h')
        + L._plane_fields('g') + L._plane_fields('x') + L._plane_fields('hw') + L._plane_fields('out')
    )


class FigsrInputParams(C.Structure):
    """Mirror of ``struct rsa_figsr_input_params``."""

    _fields_ = L._i32('batch', 'C', 'src_h', 'src_w', 'pad', 'dtype', 'fmt', 'reserved0') + L._ptr('x', 'shift', 'scale_norm') + L._plane_fields('out')


class FigsrOutputParams(C.Structure):
    """Mirror of ``struct rsa_figsr_output_params``."""

    _fields_ = L._i32('batch', 'C', 'H', 'W', 'y0', 'x0', 'out_h', 'out_w', 'dtype', 'reserved0') + L._ptr('y', 'shift', 'scale_norm', 'out')


SIGNATURES = {
    'rsa_figsr_mix': L._descriptor(FigsrMixParams),
    'rsa_figsr_band_packed_weight_bytes': (C.c_int64, L._i32('ksize', 'gc', 'products')),
    'rsa_figsr_input': L._descriptor(FigsrInputParams),
    'rsa_figsr_output': L._descriptor(FigsrOutputParams),
}

L.extend(SIGNATURES, 'resselt_amd_figsr.h')


def pack_band_weights(w_w: torch.Tensor, w_h: torch.Tensor, products: int, fmt: int) -> torch.Tensor:
    """The 1 x K weights ``w_w`` [gc, gc, 1, K] and the K x 1 weights ``w_h`` [gc, gc, K, 1] -> the A-fragment blob of ``rsa_figsr_mix``
    (include/resselt_amd_figsr.h), a 16-bit container tensor: [band][input plane p][step s][half][lane = 16 tap-in-step + cout16][8 input
    channels], zero past K and past output channel gc."""
    gc, cin, _, k = w_w.shape
    if gc != cin or gc not in (8, 16) or tuple(w_w.shape) != (gc, gc, 1, k) or tuple(w_h.shape) != (gc, gc, k, 1):
        raise ValueError(f'band weights must be [gc, gc, 1, K] and [gc, gc, K, 1] with gc 8 or 16, got {tuple(w_w.shape)} and {tuple(w_h.shape)}')
    P, S = gc // 8, (k + 3) // 4
    wt = torch.zeros((2, 16, gc, S * 4), dtype=torch.float32, device=w_w.device)
    wt[0, :gc, :, :k] = w_w.to(torch.float32).reshape(gc, gc, k)
    wt[1, :gc, :, :k] = w_h.to(torch.float32).reshape(gc, gc, k)
    # [band][cout16][p][j][s][grp] -> [band][p][s][grp][cout16][j]: lane = 16 grp + cout16
    wt = wt.reshape(2, 16, P, 8, S, 4).permute(0, 2, 4, 5, 1, 3).reshape(2, P, S, 1, 64, 8)
    dt = torch.float16 if fmt == PF_F16 else torch.bfloat16
    hi = wt.to(dt)
    parts = [hi]
    if int(products) == 3:
        parts.append((wt - hi.to(torch.float32)).to(dt))
    blob = torch.cat(parts, dim=3).contiguous().view(torch.bfloat16).reshape(-1)
    nbytes = int(L.load().rsa_figsr_band_packed_weight_bytes(k, gc, int(products)))
    if blob.numel() * 2 != nbytes:
        raise AssertionError(f'band blob is {blob.numel() * 2} bytes, the library expects {nbytes}')
    return blob


def band_bias(b: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(16, dtype=torch.float32, device=b.device)
    out[: b.numel()] = b.to(torch.float32)
    return out
