"""include/resselt_amd_gfisr1.h against its ctypes mirrors and signature rows (resselt_amd/engine/lib_gfisr1.py): the same structs with the
same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, and the argument checks that need no GPU.  The parsers are those of tests/test_moesr_capi.py, pointed at this header."""

import ctypes
import os
import re

import pytest

import test_moesr_capi as P
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gfisr1 as LG1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_gfisr1.h')
MIRRORS = {'rsa_gfisr_ln_spectral_params': LG1.GfisrLnSpectralParams, 'rsa_plane_window_params': LG1.PlaneWindowParams}
E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3


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
    assert ctypes.sizeof(LG1.GfisrLnSpectralParams) == 6 * 4 + 8 * 8  # no padding: the C compiler lays it out the same way
    assert ctypes.sizeof(LG1.PlaneWindowParams) == 8 * 4 + 2 * (2 * 8 + 2 * 8)


def test_the_prototypes_match_their_rows(header):
    protos = P._header_prototypes()
    assert list(protos) == list(LG1.SIGNATURES) == ['rsa_gfisr_ln_spectral', 'rsa_plane_window']
    names = {ctypes.POINTER(LG1.GfisrLnSpectralParams): 'rsa_gfisr_ln_spectral_params', ctypes.POINTER(LG1.PlaneWindowParams): 'rsa_plane_window_params',
             ctypes.c_void_p: 'ptr'}  # fmt: skip
    for entry, (restype, params) in LG1.SIGNATURES.items():
        assert restype is ctypes.c_int and protos[entry][0] == 'int', entry
        assert [(k, names[t]) for k, t in params] == protos[entry][1], entry


def test_the_main_tables_do_not_know_them_and_the_library_does():
    from resselt_amd.engine import lib_gfisr as LG

    for entry, row in LG1.SIGNATURES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS and entry not in LG.SIGNATURES
        assert L.EXTENSIONS[entry] is row and L.signature(entry) is row
    assert '#include "resselt_amd.h"' in open(HEADER).read()
    lib = L.load()
    for entry, (restype, params) in LG1.SIGNATURES.items():
        fn = getattr(lib, entry)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params]


def _err(lib):
    return lib.rsa_last_error_string()


def test_ln_spectral_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_gfisr_ln_spectral(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG1.GfisrLnSpectralParams()
    assert lib.rsa_gfisr_ln_spectral(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.eps = 1, 4, 4, 12, 1e-6
    for key, bad in (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('eps', 0.0)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert lib.rsa_gfisr_ln_spectral(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    for c in (1, 3, 31, 33, 34, 64):
        p.C = c
        assert lib.rsa_gfisr_ln_spectral(ctypes.byref(p), None) == E_UNSUPPORTED and b'even and in 2..32' in _err(lib), c
    p.C = 12
    ptrs = ('x', 'ln_w', 'ln_b', 'fpe_w', 'fpe_b', 'fdc_w', 'fdc_b', 'out')
    for i, k in enumerate(ptrs):
        setattr(p, k, 64 * (i + 1))
    for i, k in enumerate(ptrs):
        setattr(p, k, None)
        assert lib.rsa_gfisr_ln_spectral(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib), k
        setattr(p, k, 64 * (i + 1) + 8)
        assert lib.rsa_gfisr_ln_spectral(ctypes.byref(p), None) == E_ALIGN, k
        setattr(p, k, 64 * (i + 1))
    p.out = p.x
    assert lib.rsa_gfisr_ln_spectral(ctypes.byref(p), None) == E_ARG and b'must not overlap' in _err(lib)


def test_plane_window_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_plane_window(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG1.PlaneWindowParams()
    assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.planes, p.H, p.W, p.out_H, p.out_W, p.top, p.left = 1, 2, 5, 4, 10, 8, 2, 2
    for key in ('batch', 'planes', 'H', 'W', 'out_H', 'out_W'):
        keep = getattr(p, key)
        setattr(p, key, 0)
        assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib)
    p.in_hi, p.out_hi = 64, 128
    p.in_lo = 256
    assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'go together' in _err(lib)
    p.in_lo, p.out_lo = None, 256
    assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'go together' in _err(lib)
    p.in_lo = 512
    for k in ('in_hi', 'in_lo', 'out_hi', 'out_lo'):
        keep = getattr(p, k)
        setattr(p, k, keep + 4)
        assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ALIGN, k
        setattr(p, k, keep)
    p.in_plane_stride, p.out_plane_stride = 19, 80
    assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib)
    p.in_plane_stride, p.out_plane_stride = 20, 79
    assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib)
    p.out_plane_stride = 400
    # torch's rule: a pad must stay below the side -- an index may reflect once, never twice
    for key, bad in (('top', 5), ('left', 4), ('out_H', 2 + 2 * 4 + 2), ('out_W', 2 + 2 * 3 + 2), ('top', -6), ('H', 2)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert lib.rsa_plane_window(ctypes.byref(p), None) == E_ARG and b'second reflection' in _err(lib), (key, bad)
        setattr(p, key, keep)
