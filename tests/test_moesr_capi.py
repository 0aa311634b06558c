"""The argument checks of ``rsa_moesr_stream`` (include/resselt_amd_moesr.h) that need no GPU: each returns before any launch.
tests/test_capi_headers.py compares the header with its ctypes mirror and row (resselt_amd/engine/lib_moesr.py)."""

import ctypes

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_moesr as LM


def test_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_moesr_stream(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LM.MoesrStreamParams()
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'geometry' in lib.rsa_last_error_string()
    p.batch, p.H, p.W, p.C, p.mode, p.a_H, p.a_W = 1, 4, 4, 12, 0, 4, 4
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'multiple of 8' in lib.rsa_last_error_string()
    p.C, p.mode, p.a_H = 8, 1, 7
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'odd source size' in lib.rsa_last_error_string()
    p.mode, p.a_H = 0, 4
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'null operand' in lib.rsa_last_error_string()
    p.a, p.gamma, p.s_in, p.s_out = 16, 16, 16, 24
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -3  # misaligned pointer
