"""include/resselt_amd_gfisr.h against its ctypes mirrors and signature rows (resselt_amd/engine/lib_gfisr.py): the same structs with the
same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, and the argument checks that need no GPU.  The parsers are those of tests/test_moesr_capi.py, pointed at this header."""

import ctypes
import os
import re

import pytest

import test_moesr_capi as P
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gfisr as LG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_gfisr.h')
MIRRORS = {'rsa_gfisr_dft_params': LG.GfisrDftParams, 'rsa_gfisr_spectral_params': LG.GfisrSpectralParams}


@pytest.fixture
def header(monkeypatch):
    text = open(HEADER).read()
    monkeypatch.setattr(P, '_header', lambda: re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))


def test_the_structs_match_their_mirrors(header):
    structs = P._header_structs()
    assert list(structs) == list(MIRRORS)
    classes = {ctypes.c_int32: 'int32_t', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float', ctypes.c_void_p: 'pointer'}
    for name, mirror in MIRRORS.items():
        assert name in mirror.__doc__
        assert [(k, classes[t]) for k, t in mirror._fields_] == structs[name]
    assert ctypes.sizeof(LG.GfisrDftParams) == 8 * 4 + 8 * 8 + 2 * 8  # no padding: the C compiler lays it out the same way
    assert ctypes.sizeof(LG.GfisrSpectralParams) == 6 * 4 + 7 * 8 + 2 * 8


def test_the_prototypes_match_their_rows(header):
    protos = P._header_prototypes()
    assert list(protos) == list(LG.SIGNATURES) == ['rsa_gfisr_dft', 'rsa_gfisr_dft_scratch_bytes', 'rsa_gfisr_spectral', 'rsa_gfisr_gate']
    names = {ctypes.POINTER(LG.GfisrDftParams): 'rsa_gfisr_dft_params', ctypes.POINTER(LG.GfisrSpectralParams): 'rsa_gfisr_spectral_params',
             ctypes.POINTER(L.GatedDwConvParams): 'rsa_gated_dwconv_params', ctypes.c_void_p: 'ptr', ctypes.c_int32: 'int32_t'}  # fmt: skip
    rets = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t'}
    for entry, (restype, params) in LG.SIGNATURES.items():
        assert rets[restype] == protos[entry][0], entry
        assert [(k, names[t]) for k, t in params] == protos[entry][1], entry
    assert LG.SIGNATURES['rsa_gfisr_gate'][1][0][1] is L.SIGNATURES['rsa_gated_dwconv'][1][0][1]  # rsa_gated_dwconv_params, unchanged


def test_the_main_tables_do_not_know_them_and_the_library_does():
    for entry, row in LG.SIGNATURES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS and L.EXTENSIONS[entry] is row and L.signature(entry) is row
    assert L.signature('rsa_gated_dwconv') is L.SIGNATURES['rsa_gated_dwconv']
    assert '#include "resselt_amd.h"' in open(HEADER).read()
    lib = L.load()
    for entry, (restype, params) in LG.SIGNATURES.items():
        fn = getattr(lib, entry)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params]


def test_keyword_binding_reaches_an_extension_entry_point():
    gp = L.GatedDwConvParams()
    argv = L.bind('rsa_gfisr_gate', p=gp, act=L.ACT_SILU)
    assert argv == [gp, L.ACT_SILU]
    with pytest.raises(TypeError, match="missing parameter 'act'"):
        L.bind('rsa_gfisr_gate', p=gp)


def _err(lib):
    return lib.rsa_last_error_string()


def test_dft_argument_validation_without_gpu():
    lib = L.load()
    E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3
    assert lib.rsa_gfisr_dft(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG.GfisrDftParams()
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C = 1, 4, 6, 10
    for key, bad in (('inverse', 2), ('reserved0', 1), ('batch', 0), ('H', 0), ('W', 0), ('C', 0)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    p.C = 129
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_UNSUPPORTED and b'1..128' in _err(lib)
    p.C, p.H = 10, 40000
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_UNSUPPORTED and b'too large' in _err(lib)
    p.H, p.fmt = 4, 2
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'plane format' in _err(lib)
    p.fmt = 0
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib)
    ptrs = ('tab_row', 'tab_col', 'spec', 'scratch', 'plane_hi')
    for k in ptrs:
        setattr(p, k, 64)
    for k in ptrs:
        setattr(p, k, None)
        assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib), k
        setattr(p, k, 64)
    p.inverse, p.norm_scale = 1, 64
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'norm_offset and eps' in _err(lib)
    p.norm_offset = 64
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'norm_offset and eps' in _err(lib)  # eps = 0
    p.eps = 1e-6
    for k in ptrs + ('plane_lo', 'norm_scale', 'norm_offset'):
        keep = getattr(p, k)
        setattr(p, k, 68)
        assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ALIGN, k
        setattr(p, k, keep)
    p.plane_plane_stride = 23
    assert lib.rsa_gfisr_dft(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib)
    assert lib.rsa_gfisr_dft_scratch_bytes(2, 10, 5, 7) == 2 * 10 * (2 * 5 * 4 + 5 * 7) * 4
    for bad in ((0, 10, 5, 7), (1, 0, 5, 7), (1, 129, 5, 7), (1, 10, 0, 7), (1, 10, 5, 0), (1, 10, 40000, 7)):
        assert lib.rsa_gfisr_dft_scratch_bytes(*bad) == -1, bad


def test_spectral_argument_validation_without_gpu():
    lib = L.load()
    E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3
    assert lib.rsa_gfisr_spectral(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG.GfisrSpectralParams()
    assert lib.rsa_gfisr_spectral(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.eps = 1, 4, 4, 20, 1e-6
    for key, bad in (('reserved0', 1), ('batch', 0), ('H', 0), ('W', 0), ('C', 0), ('eps', 0.0)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert lib.rsa_gfisr_spectral(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    p.C = 257
    assert lib.rsa_gfisr_spectral(ctypes.byref(p), None) == E_UNSUPPORTED and b'1..256' in _err(lib)
    p.C = 20
    ptrs = ('x', 'scale', 'offset', 'weight', 'bias', 'out_hi')
    for k in ptrs:
        setattr(p, k, 64)
    for k in ptrs:
        setattr(p, k, None)
        assert lib.rsa_gfisr_spectral(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib), k
        setattr(p, k, 64)
    for k in ptrs + ('out_lo',):
        keep = getattr(p, k)
        setattr(p, k, 72)
        assert lib.rsa_gfisr_spectral(ctypes.byref(p), None) == E_ALIGN, k
        setattr(p, k, keep)
    p.out_plane_stride = 15
    assert lib.rsa_gfisr_spectral(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib)


def test_gate_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_gfisr_gate(None, L.ACT_SILU, None) == -1 and b'null params' in _err(lib)
    p = L.GatedDwConvParams()
    assert lib.rsa_gfisr_gate(ctypes.byref(p), L.ACT_GELU, None) == -2 and b'RSA_ACT_MISH or RSA_ACT_SILU' in _err(lib)
    for act in (L.ACT_MISH, L.ACT_SILU):  # then every check of rsa_gated_dwconv, in its words
        assert lib.rsa_gfisr_gate(ctypes.byref(p), act, None) == -1 and b'gated_dwconv: bad geometry' in _err(lib)
    p.batch, p.H, p.W, p.i_planes, p.n_segments = 1, 4, 4, 1, 1
    p.seg[0].planes, p.seg[0].kh, p.seg[0].kw = 1, 3, 5
    assert lib.rsa_gfisr_gate(ctypes.byref(p), L.ACT_SILU, None) == -2 and b'tap shape not compiled' in _err(lib)
