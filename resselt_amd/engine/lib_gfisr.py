"""ctypes mirrors and signature rows of include/resselt_amd_gfisr.h (``rsa_gfisr_dft``, ``rsa_gfisr_dft_scratch_bytes``,
``rsa_gfisr_spectral``, ``rsa_gfisr_gate``; csrc/gfisr.hip and csrc/mosr.hip), registered with ``lib.extend``, and the host-side builder of
the DFT tables ``rsa_gfisr_dft`` multiplies with.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirrors and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as L


class GfisrDftParams(C.Structure):
    """Mirror of ``struct rsa_gfisr_dft_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'inverse', 'fmt') + L._f32('eps') + L._i32('reserved0')
        + L._ptr('tab_row', 'tab_col', 'spec', 'scratch', 'norm_scale', 'norm_offset') + L._plane_fields('plane')
    )


class GfisrSpectralParams(C.Structure):
    """Mirror of ``struct rsa_gfisr_spectral_params``."""

    _fields_ = L._i32('batch', 'H', 'W', 'C') + L._f32('eps') + L._i32('reserved0') + L._ptr('x', 'scale', 'offset', 'weight', 'bias') + L._plane_fields('out')


SIGNATURES = {
    'rsa_gfisr_dft': L._descriptor(GfisrDftParams),
    'rsa_gfisr_dft_scratch_bytes': (C.c_int64, L._i32('batch', 'C', 'H', 'W')),
    'rsa_gfisr_spectral': L._descriptor(GfisrSpectralParams),
    'rsa_gfisr_gate': (C.c_int, [('p', C.POINTER(L.GatedDwConvParams))] + L._i32('act') + L._ptr('stream')),
}

L.extend(SIGNATURES, 'resselt_amd_gfisr.h')


def _angles(a: np.ndarray, b: np.ndarray, n: int) -> np.ndarray:
    """2 pi ((a b) mod n) / n for index vectors a, b: the product is reduced as an integer before the angle is taken."""
    return (2.0 * np.pi / n) * ((a[:, None].astype(np.int64) * b[None, :].astype(np.int64)) % n).astype(np.float64)


def dft_tables_f64(H: int, W: int) -> dict:
    """The four DFT tables of ``rsa_gfisr_dft`` in float64 (the layouts resselt_amd_gfisr.h gives), the ortho factor folded in:
    ``row_fwd`` [W, 2 Wf], ``row_inv`` [2 Wf, W] with irfft2's column weights c_k, ``col_fwd`` / ``col_inv`` [2H, 2H] k-major."""
    Wf = W // 2 + 1
    th = _angles(np.arange(W), np.arange(Wf), W)  # [x, k]
    row_fwd = np.concatenate([np.cos(th), -np.sin(th)], 1) / np.sqrt(W)
    ck = np.full(Wf, 2.0)
    ck[0] = 1.0
    if W % 2 == 0:
        ck[W // 2] = 1.0
    row_inv = np.concatenate([ck[:, None] * np.cos(th.T), -ck[:, None] * np.sin(th.T)], 0) / np.sqrt(W)
    tv = _angles(np.arange(H), np.arange(H), H)  # [v, y], symmetric
    c, s = np.cos(tv) / np.sqrt(H), np.sin(tv) / np.sqrt(H)
    g = np.block([[c, s], [-s, c]])  # [re; im] of the forward column transform = G [re; im]
    # k-major storage: the kernel reads A[m][k] at [k][m], so the forward table is G transposed and the inverse one (G^T) is G itself
    return dict(row_fwd=row_fwd, row_inv=row_inv, col_fwd=np.ascontiguousarray(g.T), col_inv=g)


def rfft2_f64(x: torch.Tensor) -> torch.Tensor:
    """rfft2(norm='ortho') of a real float64 [..., H, W] tensor through the float64 tables: [..., 2, H, Wf] (real, imaginary)."""
    H, W = x.shape[-2:]
    Wf = W // 2 + 1
    t = {k: torch.from_numpy(v) for k, v in dft_tables_f64(H, W).items()}
    r = x @ t['row_fwd']  # [..., H, 2 Wf]
    stacked = torch.cat([r[..., :Wf], r[..., Wf:]], -2)  # [..., 2H, Wf]
    z = t['col_fwd'].T @ stacked
    return torch.stack([z[..., :H, :], z[..., H:, :]], -3)


def irfft2_f64(z: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """irfft2(s=(H, W), norm='ortho') of a half spectrum [..., 2, H, Wf] (real, imaginary; need not be Hermitian) through the tables."""
    t = {k: torch.from_numpy(v) for k, v in dft_tables_f64(H, W).items()}
    stacked = torch.cat([z[..., 0, :, :], z[..., 1, :, :]], -2)  # [..., 2H, Wf]
    y = t['col_inv'].T @ stacked
    return torch.cat([y[..., :H, :], y[..., H:, :]], -1) @ t['row_inv']


def dft_tables(H: int, W: int, device) -> dict:
    """The tables rounded once to f32, on ``device``."""
    return {k: torch.from_numpy(v.astype(np.float32)).contiguous().to(device) for k, v in dft_tables_f64(H, W).items()}
