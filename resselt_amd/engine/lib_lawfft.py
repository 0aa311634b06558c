"""ctypes mirrors and signature rows of include/resselt_amd_lawfft.h (``rsa_lawfft_wincorr``, ``rsa_lawfft_spec_mul``,
``rsa_lawfft_norm_mul``, ``rsa_lawfft_kernel_gen``, ``rsa_lawfft_kernel_gen_workspace_bytes``, ``rsa_lawfft_dyn_dwconv``;
csrc/lawfft.hip), registered with ``lib.extend``, and the host-side layout of the kernel generator's two matrices.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirrors and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import lib as L


class LawfftWincorrParams(C.Structure):
    """Mirror of ``struct rsa_lawfft_wincorr_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'fmt', 'reserved0') + L._f32('eps') + L._i32('reserved1') + L._ptr('weight', 'bias')
        + L._plane_fields('q') + L._plane_fields('k') + L._plane_fields('v') + L._plane_fields('out')
    )


class LawfftSpecMulParams(C.Structure):
    """Mirror of ``struct rsa_lawfft_spec_mul_params``."""

    _fields_ = L._i32('batch', 'H', 'W', 'C') + L._f32('scale') + L._i32('reserved0') + L._ptr('a', 'b', 'out')


class LawfftNormMulParams(C.Structure):
    """Mirror of ``struct rsa_lawfft_norm_mul_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'corr_fmt', 'fmt') + L._f32('eps') + L._i32('reserved0') + L._ptr('weight', 'bias')
        + L._plane_fields('corr') + L._plane_fields('v') + L._plane_fields('out')
    )


class LawfftKernelGenParams(C.Structure):
    """Mirror of ``struct rsa_lawfft_kernel_gen_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'ksize', 'fmt', 'reserved0', 'reserved1') + L._ptr('w1_t', 'b1', 'w2_t', 'b2', 'workspace', 'out')
        + L._plane_fields('in')
    )


class LawfftDynDwConvParams(C.Structure):
    """Mirror of ``struct rsa_lawfft_dyn_dwconv_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'ksize', 'fmt', 'reserved0', 'reserved1') + L._ptr('weight', 'res1', 'res2', 'out_f32')
        + L._plane_fields('in') + L._plane_fields('out')
    )


SIGNATURES = {
    'rsa_lawfft_wincorr': L._descriptor(LawfftWincorrParams),
    'rsa_lawfft_spec_mul': L._descriptor(LawfftSpecMulParams),
    'rsa_lawfft_norm_mul': L._descriptor(LawfftNormMulParams),
    'rsa_lawfft_kernel_gen': L._descriptor(LawfftKernelGenParams),
    'rsa_lawfft_kernel_gen_workspace_bytes': (C.c_int64, L._i32('batch', 'C', 'H', 'W')),
    'rsa_lawfft_dyn_dwconv': L._descriptor(LawfftDynDwConvParams),
}

L.extend(SIGNATURES, 'resselt_amd_lawfft.h')


def pack_kernel_gen(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """DynamicLocal's two 1x1 convolutions ``kernel_gen.1`` [C, C, 1, 1] and ``kernel_gen.3`` [C k^2, C, 1, 1] -> (w1_t [C, C], b1 [C],
    w2_t [C, C k^2], b2 [C k^2]) f32: the matrices transposed, so that the threads of ``rsa_lawfft_kernel_gen`` read consecutive words."""
    c = w1.shape[0]
    if tuple(w1.shape[:2]) != (c, c) or w2.shape[1] != c or w2.shape[0] % c:
        raise ValueError(f'kernel_gen weights must be [C, C, 1, 1] and [C k^2, C, 1, 1], got {tuple(w1.shape)} and {tuple(w2.shape)}')
    f32 = torch.float32
    return (w1.reshape(c, c).t().to(f32).contiguous(), b1.to(f32).contiguous(), w2.reshape(-1, c).t().to(f32).contiguous(), b2.to(f32).contiguous())
