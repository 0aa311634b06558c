"""ctypes mirrors and signature rows of include/resselt_amd_smosr.h (``rsa_smosr_gate``, ``rsa_smosr_pad``, ``rsa_smosr_pa``;
csrc/smosr.hip), registered with ``lib.extend``, and the host-side packing of ``rsa_smosr_pa``'s weight fragments.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirrors and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import lib as L
from .pack import split_halves
from .tensors import _PF_DTYPE


class SmosrGateParams(C.Structure):
    """Mirror of ``struct rsa_smosr_gate_params``."""

    _fields_ = L._i32('batch', 'H', 'W', 'C', 'fmt', 'reserved0') + L._ptr('a', 's_in', 's2_in', 's_out') + L._plane_fields('out')


class SmosrPadParams(C.Structure):
    """Mirror of ``struct rsa_smosr_pad_params``."""

    _fields_ = L._i32('batch', 'C', 'src_h', 'src_w', 'pad', 'dtype', 'fmt', 'reserved0') + L._ptr('x') + L._plane_fields('out')


class SmosrPaParams(C.Structure):
    """Mirror of ``struct rsa_smosr_pa_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'fmt', 'products') + L._f32('slope') + L._i32('reserved0') + L._ptr('w_frag', 'bias')
        + L._plane_fields('in') + L._plane_fields('out')
    )


SIGNATURES = {
    'rsa_smosr_gate': L._descriptor(SmosrGateParams),
    'rsa_smosr_pad': L._descriptor(SmosrPadParams),
    'rsa_smosr_pa': L._descriptor(SmosrPaParams),
}

L.extend(SIGNATURES, 'resselt_amd_smosr.h')


def pack_pa_weights(w: torch.Tensor, b: torch.Tensor, products: int, fmt: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """``w`` [C, C] (or [C, C, 1, 1]) and ``b`` [C] of a pixel attention's 1x1 convolution -> (``w_frag``, ``bias``) of ``rsa_smosr_pa``:
    A fragments [K][K][2][halves][64][8] in the 16-bit format ``fmt`` (the order resselt_amd_smosr.h gives) and the f32 bias padded to 32 K."""
    c = w.shape[0]
    w = w.detach().reshape(c, c).to(device='cpu', dtype=torch.float32)
    k = (c + 31) // 32
    wp = torch.zeros((32 * k, 32 * k), dtype=torch.float32)
    wp[:c, :c] = w
    lane = torch.arange(64)
    row, q = lane & 15, lane >> 4
    frag = torch.empty((k, k, 2, 64, 8), dtype=torch.float32)
    for mo in range(k):
        for t in range(2):
            out_ch = 32 * mo + 8 * (row >> 2) + 4 * t + (row & 3)  # [64]
            for ki in range(k):
                in_ch = 32 * ki + 8 * q[:, None] + torch.arange(8)[None, :]  # [64, 8]
                frag[mo, ki, t] = wp[out_ch[:, None], in_ch]
    hi, lo = split_halves(frag, _PF_DTYPE[fmt])
    halves = torch.stack([hi, lo], 3) if int(products) == 3 else hi.unsqueeze(3)  # [K][K][2][halves][64][8]
    bias = torch.zeros(32 * k, dtype=torch.float32)
    bias[:c] = b.detach().to(device='cpu', dtype=torch.float32)
    return halves.contiguous().to(device), bias.to(device)
