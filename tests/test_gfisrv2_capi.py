"""The argument checks of ``rsa_gfisr_dft``, ``rsa_gfisr_spectral`` and ``rsa_gfisr_gate`` (include/resselt_amd_gfisr.h) that need no GPU
(each returns before any launch), the scratch size, and the keyword binder on an extension's row.  tests/test_capi_headers.py compares
the header with its ctypes mirrors and rows (resselt_amd/engine/lib_gfisr.py)."""

import ctypes

import pytest

import capi_header as H
from capi_header import E_ALIGN, E_ARG, E_UNSUPPORTED, err
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gfisr as LG


def test_keyword_binding_reaches_an_extension_entry_point():
    gp = L.GatedDwConvParams()
    argv = L.bind('rsa_gfisr_gate', p=gp, act=L.ACT_SILU)
    assert argv == [gp, L.ACT_SILU]
    with pytest.raises(TypeError, match="missing parameter 'act'"):
        L.bind('rsa_gfisr_gate', p=gp)


def test_dft_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_gfisr_dft(None, None) == E_ARG and b'null params' in err(lib)
    p = LG.GfisrDftParams()
    call = H.caller(lib.rsa_gfisr_dft, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C = 1, 4, 6, 10
    H.each_bad(lib, call, p, (('inverse', 2), ('reserved0', 1), ('batch', 0), ('H', 0), ('W', 0), ('C', 0)), E_ARG, b'geometry')
    p.C = 129
    assert call() == E_UNSUPPORTED and b'1..128' in err(lib)
    p.C, p.H = 10, 40000
    assert call() == E_UNSUPPORTED and b'too large' in err(lib)
    p.H, p.fmt = 4, 2
    assert call() == E_ARG and b'plane format' in err(lib)
    p.fmt = 0
    assert call() == E_ARG and b'null pointer' in err(lib)
    ptrs = ('tab_row', 'tab_col', 'spec', 'scratch', 'plane_hi')
    for k in ptrs:
        setattr(p, k, 64)
    H.each_null(lib, call, p, ptrs, b'null pointer')
    p.inverse, p.norm_scale = 1, 64
    assert call() == E_ARG and b'norm_offset and eps' in err(lib)
    p.norm_offset = 64
    assert call() == E_ARG and b'norm_offset and eps' in err(lib)  # eps = 0
    p.eps = 1e-6
    H.each_misaligned(lib, call, p, ptrs + ('plane_lo', 'norm_scale', 'norm_offset'), at=68)
    p.plane_plane_stride = 23
    assert call() == E_ARG and b'plane stride' in err(lib)
    assert lib.rsa_gfisr_dft_scratch_bytes(2, 10, 5, 7) == 2 * 10 * (2 * 5 * 4 + 5 * 7) * 4
    for bad in ((0, 10, 5, 7), (1, 0, 5, 7), (1, 129, 5, 7), (1, 10, 0, 7), (1, 10, 5, 0), (1, 10, 40000, 7)):
        assert lib.rsa_gfisr_dft_scratch_bytes(*bad) == -1, bad


def test_spectral_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_gfisr_spectral(None, None) == E_ARG and b'null params' in err(lib)
    p = LG.GfisrSpectralParams()
    call = H.caller(lib.rsa_gfisr_spectral, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.eps = 1, 4, 4, 20, 1e-6
    H.each_bad(lib, call, p, (('reserved0', 1), ('batch', 0), ('H', 0), ('W', 0), ('C', 0), ('eps', 0.0)), E_ARG, b'geometry')
    p.C = 257
    assert call() == E_UNSUPPORTED and b'1..256' in err(lib)
    p.C = 20
    ptrs = ('x', 'scale', 'offset', 'weight', 'bias', 'out_hi')
    for k in ptrs:
        setattr(p, k, 64)
    H.each_null(lib, call, p, ptrs, b'null pointer')
    H.each_misaligned(lib, call, p, ptrs + ('out_lo',), at=72)
    p.out_plane_stride = 15
    assert call() == E_ARG and b'plane stride' in err(lib)


def test_gate_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_gfisr_gate(None, L.ACT_SILU, None) == -1 and b'null params' in err(lib)
    p = L.GatedDwConvParams()
    assert lib.rsa_gfisr_gate(ctypes.byref(p), L.ACT_GELU, None) == -2 and b'RSA_ACT_MISH or RSA_ACT_SILU' in err(lib)
    for act in (L.ACT_MISH, L.ACT_SILU):  # then every check of rsa_gated_dwconv, in its words
        assert lib.rsa_gfisr_gate(ctypes.byref(p), act, None) == -1 and b'gated_dwconv: bad geometry' in err(lib)
    p.batch, p.H, p.W, p.i_planes, p.n_segments = 1, 4, 4, 1, 1
    p.seg[0].planes, p.seg[0].kh, p.seg[0].kw = 1, 3, 5
    assert lib.rsa_gfisr_gate(ctypes.byref(p), L.ACT_SILU, None) == -2 and b'tap shape not compiled' in err(lib)
