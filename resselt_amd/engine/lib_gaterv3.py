"""ctypes mirrors and signature rows of include/resselt_amd_gaterv3.h (``rsa_gaterv3_local_gate``, ``rsa_gaterv3_sca_apply``,
``rsa_gaterv3_channel_attention``, ``rsa_gaterv3_shortcut`` and the two workspace sizes; csrc/gaterv3.hip), registered with ``lib.extend``.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirrors and the rows with the header.
"""

from __future__ import annotations

import ctypes as C

from . import lib as L

TILE_W, TILE_H = 32, 8  # RSA_GATERV3_TILE_W / _H: the reduction chunk of rsa_gaterv3_local_gate
TOKEN_CHUNK = 128  # RSA_GATERV3_TOKEN_CHUNK: the reduction chunk of rsa_gaterv3_channel_attention


class LocalGateParams(C.Structure):
    """Mirror of ``struct rsa_gaterv3_local_gate_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'dim', 'fmt', 'reserved0') + L._plane_fields('x') + L._ptr('weight', 'bias') + L._plane_fields('out')
        + L._ptr('workspace') + L._i64('workspace_bytes')
    )


class ScaApplyParams(C.Structure):
    """Mirror of ``struct rsa_gaterv3_sca_apply_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'dim', 'fmt', 'reserved0') + L._plane_fields('s') + L._ptr('sca_w', 'sca_b', 'gamma0', 'short_f32', 'out_f32')
        + L._ptr('workspace') + L._i64('workspace_bytes')
    )


class AttnParams(C.Structure):
    """Mirror of ``struct rsa_gaterv3_attn_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'heads', 'head_dim', 'fmt', 'reserved0') + L._plane_fields('qkv') + L._ptr('temperature')
        + L._plane_fields('out') + L._ptr('workspace') + L._i64('workspace_bytes')
    )


class ShortcutParams(C.Structure):
    """Mirror of ``struct rsa_gaterv3_shortcut_params``."""

    _fields_ = L._i32('batch', 'C', 'h', 'w', 'scale', 'out_H', 'out_W', 'dtype') + L._ptr('x', 'gamma', 'out')


SIGNATURES = {
    'rsa_gaterv3_local_workspace_bytes': (C.c_int64, L._i32('batch', 'H', 'W', 'dim')),
    'rsa_gaterv3_local_gate': L._descriptor(LocalGateParams),
    'rsa_gaterv3_sca_apply': L._descriptor(ScaApplyParams),
    'rsa_gaterv3_attn_workspace_bytes': (C.c_int64, L._i32('batch', 'H', 'W', 'heads', 'head_dim')),
    'rsa_gaterv3_channel_attention': L._descriptor(AttnParams),
    'rsa_gaterv3_shortcut': L._descriptor(ShortcutParams),
}

L.extend(SIGNATURES, 'resselt_amd_gaterv3.h')
