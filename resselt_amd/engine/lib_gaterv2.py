"""ctypes mirror and signature rows of include/resselt_amd_gaterv2.h (``rsa_gaterv2_linear_attention`` and its workspace size;
csrc/gaterv2.hip), registered with ``lib.extend``.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirror and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

from . import lib as L

TOKEN_CHUNK = 128  # RSA_GATERV2_TOKEN_CHUNK: the reduction chunk of rsa_gaterv2_linear_attention


class AttnParams(C.Structure):
    """Mirror of ``struct rsa_gaterv2_attn_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'm', 'fmt') + L._f32('eps') + L._i32('reserved0') + L._plane_fields('qkv') + L._plane_fields('out')
        + L._ptr('workspace') + L._i64('workspace_bytes')
    )


SIGNATURES = {
    'rsa_gaterv2_attn_workspace_bytes': (C.c_int64, L._i32('batch', 'H', 'W', 'C', 'm')),
    'rsa_gaterv2_linear_attention': L._descriptor(AttnParams),
}

L.extend(SIGNATURES, 'resselt_amd_gaterv2.h')


def record_floats(c: int, m: int) -> int:
    """One record [M m x C | ksum m | vsum C] of the workspace, in f32 values."""
    return m * c + m + c
