"""ctypes mirrors and signature rows of include/resselt_amd_gfisr1.h (``rsa_gfisr_ln_spectral``, ``rsa_plane_window``; csrc/gfisr1.hip),
registered with ``lib.extend``.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirrors and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

from . import lib as L


class GfisrLnSpectralParams(C.Structure):
    """Mirror of ``struct rsa_gfisr_ln_spectral_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C') + L._f32('eps') + L._i32('reserved0')
        + L._ptr('x', 'ln_w', 'ln_b', 'fpe_w', 'fpe_b', 'fdc_w', 'fdc_b', 'out')
    )


class PlaneWindowParams(C.Structure):
    """Mirror of ``struct rsa_plane_window_params``."""

    _fields_ = L._i32('batch', 'planes', 'H', 'W', 'out_H', 'out_W', 'top', 'left') + L._plane_fields('in') + L._plane_fields('out')


SIGNATURES = {
    'rsa_gfisr_ln_spectral': L._descriptor(GfisrLnSpectralParams),
    'rsa_plane_window': L._descriptor(PlaneWindowParams),
}

L.extend(SIGNATURES, 'resselt_amd_gfisr1.h')
