"""include/resselt_amd_lawfft.h against its ctypes mirrors and signature rows (resselt_amd/engine/lib_lawfft.py): the same structs with
the same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, and the argument checks of every entry point that need no GPU (each returns before any launch).  The parsers are those of
tests/test_moesr_capi.py, pointed at this header."""

import ctypes
import os
import re

import pytest
import torch

import test_moesr_capi as P
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_figsr as LF
from resselt_amd.engine import lib_gfisr as LG
from resselt_amd.engine import lib_lawfft as LW
from resselt_amd.engine.tensors import PF_BF16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_lawfft.h')
MIRRORS = {'rsa_lawfft_wincorr_params': LW.LawfftWincorrParams, 'rsa_lawfft_spec_mul_params': LW.LawfftSpecMulParams, 'rsa_lawfft_norm_mul_params': LW.LawfftNormMulParams,
           'rsa_lawfft_kernel_gen_params': LW.LawfftKernelGenParams, 'rsa_lawfft_dyn_dwconv_params': LW.LawfftDynDwConvParams}  # fmt: skip
ENTRIES = ['rsa_lawfft_wincorr', 'rsa_lawfft_spec_mul', 'rsa_lawfft_norm_mul', 'rsa_lawfft_kernel_gen', 'rsa_lawfft_kernel_gen_workspace_bytes', 'rsa_lawfft_dyn_dwconv']
SIZES = {'rsa_lawfft_wincorr_params': 8 * 4 + 2 * 8 + 4 * 4 * 8, 'rsa_lawfft_spec_mul_params': 6 * 4 + 3 * 8, 'rsa_lawfft_norm_mul_params': 8 * 4 + 2 * 8 + 3 * 4 * 8,
         'rsa_lawfft_kernel_gen_params': 8 * 4 + 6 * 8 + 4 * 8, 'rsa_lawfft_dyn_dwconv_params': 8 * 4 + 4 * 8 + 2 * 4 * 8}  # fmt: skip
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
        assert [(k, classes[t]) for k, t in mirror._fields_] == structs[name], name
        assert ctypes.sizeof(mirror) == SIZES[name], name  # no padding: the C compiler lays it out the same way


def test_the_prototypes_match_their_rows(header):
    protos = P._header_prototypes()
    assert list(protos) == list(LW.SIGNATURES) == ENTRIES
    names = {ctypes.POINTER(m): n for n, m in MIRRORS.items()}
    names.update({ctypes.c_void_p: 'ptr', ctypes.c_int32: 'int32_t'})
    rets = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t'}
    for entry, (restype, params) in LW.SIGNATURES.items():
        assert rets[restype] == protos[entry][0], entry
        assert [(k, names[t]) for k, t in params] == protos[entry][1], entry


def test_the_main_tables_do_not_know_them_and_the_library_does():
    for entry, row in LW.SIGNATURES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS and L.EXTENSIONS[entry] is row and L.signature(entry) is row
        assert entry not in LG.SIGNATURES and entry not in LF.SIGNATURES  # the older headers keep their names
    assert '#include "resselt_amd.h"' in open(HEADER).read()
    for other in ('resselt_amd.h', 'resselt_amd_gfisr.h', 'resselt_amd_figsr.h'):
        assert 'lawfft' not in open(os.path.join(ROOT, 'include', other)).read()
    lib = L.load()
    for entry, (restype, params) in LW.SIGNATURES.items():
        fn = getattr(lib, entry)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params]


def _err(lib):
    return lib.rsa_last_error_string()


def _geometry(lib, call, p, keys):
    """Zero or negative sizes, a batch past the grid's limit and every reserved field: RSA_E_ARG, and the message says geometry."""
    for key, bad in keys:
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert call() == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)


def _operands(lib, call, p, ptrs, what=b"null operand"):
    """Every required pointer NULL in turn: RSA_E_ARG; every plane or map pointer off a 16-byte boundary: RSA_E_ALIGN."""
    for i, k in enumerate(ptrs):
        setattr(p, k, 1024 * (i + 1))
    for k in ptrs:
        keep = getattr(p, k)
        setattr(p, k, None)
        assert call() == E_ARG and what in _err(lib), k
        setattr(p, k, keep)


def _aligned(lib, call, p, keys):
    for k in keys:
        keep = getattr(p, k)
        setattr(p, k, (1 << 21) + 8)
        assert call() == E_ALIGN and b'16-byte aligned' in _err(lib), k
        setattr(p, k, keep)


def test_wincorr_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_wincorr(None, None) == E_ARG and b'null params' in _err(lib)
    p = LW.LawfftWincorrParams()
    call = lambda: lib.rsa_lawfft_wincorr(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.fmt, p.eps = 1, 16, 24, 45, PF_BF16, 1e-6
    _geometry(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1), ('reserved1', 1)))
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in _err(lib)
    p.fmt = PF_BF16
    for h, w in ((12, 24), (16, 20), (9, 9)):
        p.H, p.W = h, w
        assert call() == E_ARG and b'multiples of 8' in _err(lib), (h, w)
    p.H, p.W, p.C = 16, 24, 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in _err(lib)
    p.C = 128
    assert call() == E_ARG and b'null operand' in _err(lib)
    _operands(lib, call, p, ('weight', 'bias', 'q_hi', 'k_hi', 'v_hi', 'out_hi'))
    for k in ('q', 'k', 'v', 'out'):
        for q in ('q', 'k', 'v', 'out'):
            setattr(p, f'{q}_plane_stride', 16 * 24)
        setattr(p, f'{k}_plane_stride', 16 * 24 - 1)
        assert call() == E_ARG and b'plane stride' in _err(lib), k
    p.out_plane_stride = 16 * 24
    _aligned(lib, call, p, ('q_hi', 'q_lo', 'k_hi', 'k_lo', 'v_hi', 'v_lo', 'out_hi', 'out_lo'))


def test_spec_mul_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_spec_mul(None, None) == E_ARG and b'null params' in _err(lib)
    p = LW.LawfftSpecMulParams()
    call = lambda: lib.rsa_lawfft_spec_mul(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.scale = 2, 16, 13, 45, 1.0
    _geometry(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1)))
    p.C = 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in _err(lib)
    p.C = 45
    assert call() == E_ARG and b'null operand' in _err(lib)
    _operands(lib, call, p, ('a', 'b', 'out'))
    _aligned(lib, call, p, ('a', 'b', 'out'))


def test_norm_mul_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_norm_mul(None, None) == E_ARG and b'null params' in _err(lib)
    p = LW.LawfftNormMulParams()
    call = lambda: lib.rsa_lawfft_norm_mul(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.eps = 1, 9, 11, 45, 1e-6
    _geometry(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1)))
    for key in ('fmt', 'corr_fmt'):
        setattr(p, key, 2)
        assert call() == E_ARG and b'plane format' in _err(lib), key
        setattr(p, key, PF_BF16)
    p.C = 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in _err(lib)
    p.C = 45
    assert call() == E_ARG and b'null operand' in _err(lib)
    _operands(lib, call, p, ('weight', 'bias', 'corr_hi', 'v_hi', 'out_hi'))
    for k in ('corr', 'v', 'out'):
        for q in ('corr', 'v', 'out'):
            setattr(p, f'{q}_plane_stride', 99)
        setattr(p, f'{k}_plane_stride', 98)
        assert call() == E_ARG and b'plane stride' in _err(lib), k
    p.out_plane_stride = 99
    _aligned(lib, call, p, ('corr_hi', 'corr_lo', 'v_hi', 'v_lo', 'out_hi', 'out_lo'))


def test_kernel_gen_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_kernel_gen(None, None) == E_ARG and b'null params' in _err(lib)
    p = LW.LawfftKernelGenParams()
    call = lambda: lib.rsa_lawfft_kernel_gen(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.ksize = 3, 9, 11, 15, 3
    _geometry(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1), ('reserved1', 1)))
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in _err(lib)
    p.fmt, p.C = PF_BF16, 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in _err(lib)
    p.C = 15
    for k in (0, 1, 4, 7):
        p.ksize = k
        assert call() == E_UNSUPPORTED and b'ksize must be 3 or 5' in _err(lib), k
    p.ksize = 5
    assert call() == E_ARG and b'null operand' in _err(lib)
    _operands(lib, call, p, ('w1_t', 'b1', 'w2_t', 'b2', 'workspace', 'out', 'in_hi'))
    p.in_plane_stride = 98
    assert call() == E_ARG and b'plane stride' in _err(lib)
    p.in_plane_stride = 99
    _aligned(lib, call, p, ('in_hi', 'in_lo', 'workspace'))


def test_kernel_gen_workspace_bytes():
    lib = L.load()
    q = lib.rsa_lawfft_kernel_gen_workspace_bytes
    assert q(1, 1, 8, 8) == 32 and q(3, 15, 8, 8) == 3 * 2 * 32 and q(2, 60, 24, 40) == 2 * 8 * 32  # one chunk of pixels up to 4096
    assert q(1, 8, 64, 65) == 2 * 32 and q(1, 128, 512, 512) == 16 * 64 * 32 and q(1, 8, 4096, 4096) == 64 * 32  # at most 64 chunks
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 129, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0)):
        assert q(*bad) == -1, bad


def test_dyn_dwconv_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_dyn_dwconv(None, None) == E_ARG and b'null params' in _err(lib)
    p = LW.LawfftDynDwConvParams()
    call = lambda: lib.rsa_lawfft_dyn_dwconv(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.ksize = 2, 9, 11, 60, 3
    _geometry(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1), ('reserved1', 1)))
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in _err(lib)
    p.fmt = PF_BF16
    for k in (0, 1, 4, 7):
        p.ksize = k
        assert call() == E_UNSUPPORTED and b'ksize must be 3 or 5' in _err(lib), k
    p.ksize = 3
    assert call() == E_ARG and b'null operand' in _err(lib)
    _operands(lib, call, p, ('weight', 'in_hi', 'out_hi'))
    p.out_hi = None
    assert call() == E_ARG and b'null operand' in _err(lib)  # neither planes nor an f32 map to write
    p.out_lo = 4096
    p.out_f32 = 8192
    assert call() == E_ARG and b'out_lo without out_hi' in _err(lib)
    p.out_lo, p.out_hi = None, 3072
    p.in_plane_stride, p.out_plane_stride = 98, 99
    assert call() == E_ARG and b'plane stride' in _err(lib)
    p.in_plane_stride, p.out_plane_stride = 99, 98
    assert call() == E_ARG and b'plane stride' in _err(lib)
    p.out_plane_stride = 99
    keep, p.out_hi = p.out_hi, p.in_hi
    assert call() == E_ARG and b'not in place' in _err(lib)
    p.out_hi = keep
    _aligned(lib, call, p, ('in_hi', 'in_lo', 'out_hi', 'out_lo', 'res1', 'res2', 'out_f32'))


def test_pack_kernel_gen_transposes():
    c, k = 5, 3
    w1, b1 = torch.arange(c * c, dtype=torch.float32).reshape(c, c, 1, 1), torch.arange(c, dtype=torch.float32)
    w2, b2 = torch.arange(c * k * k * c, dtype=torch.float32).reshape(c * k * k, c, 1, 1), torch.arange(c * k * k, dtype=torch.float32)
    w1_t, b1_, w2_t, b2_ = LW.pack_kernel_gen(w1, b1, w2, b2)
    assert w1_t.shape == (c, c) and w2_t.shape == (c, c * k * k) and w1_t.is_contiguous() and w2_t.is_contiguous()
    assert w1_t[2, 4] == w1[4, 2, 0, 0] and w2_t[3, 17] == w2[17, 3, 0, 0] and torch.equal(b1_, b1) and torch.equal(b2_, b2)
    with pytest.raises(ValueError):
        LW.pack_kernel_gen(w1, b1, w2[:-1], b2[:-1])
