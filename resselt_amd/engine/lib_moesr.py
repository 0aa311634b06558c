"""ctypes mirror and signature row of include/resselt_amd_moesr.h (``rsa_moesr_stream``, csrc/moesr.hip), registered with ``lib.extend``.

Field order and types are the ABI; tests/test_capi_headers.py compares the mirror and the row with the header.
"""

from __future__ import annotations

import ctypes as C

from . import lib as L


class MoesrStreamParams(C.Structure):
    """Mirror of ``struct rsa_moesr_stream_params``."""

    _fields_ = (
        L._i32('batch', 'H', 'W', 'C', 'mode', 'a_H', 'a_W', 'fmt') + L._ptr('a', 'gamma', 's_in', 's2_in', 's_out', 'ln_gamma', 'ln_beta')
        + L._f32('eps') + L._i32('reserved0') + L._plane_fields('out')
    )


SIGNATURES = {'rsa_moesr_stream': L._descriptor(MoesrStreamParams)}

L.extend(SIGNATURES, 'resselt_amd_moesr.h')
