"""The argument checks of every entry point of include/resselt_amd_lawfft.h that need no GPU (each returns before any launch), the
workspace size and the kernel-generator packer.  tests/test_capi_headers.py compares the header with its ctypes mirrors and rows
(resselt_amd/engine/lib_lawfft.py)."""

import pytest
import torch

import capi_header as H
from capi_header import E_ARG, E_UNSUPPORTED, err
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_lawfft as LW
from resselt_amd.engine.tensors import PF_BF16

ALIGN = dict(at=(1 << 21) + 8, message=b'16-byte aligned')


def _operands(lib, call, p, ptrs):
    """Distinct addresses for the required pointers, then each NULL in turn."""
    H.place(p, ptrs, 1024)
    H.each_null(lib, call, p, ptrs, b'null operand')


def test_wincorr_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_wincorr(None, None) == E_ARG and b'null params' in err(lib)
    p = LW.LawfftWincorrParams()
    call = H.caller(lib.rsa_lawfft_wincorr, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.fmt, p.eps = 1, 16, 24, 45, PF_BF16, 1e-6
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1), ('reserved1', 1)), E_ARG, b'geometry')
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in err(lib)
    p.fmt = PF_BF16
    for h, w in ((12, 24), (16, 20), (9, 9)):
        p.H, p.W = h, w
        assert call() == E_ARG and b'multiples of 8' in err(lib), (h, w)
    p.H, p.W, p.C = 16, 24, 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in err(lib)
    p.C = 128
    assert call() == E_ARG and b'null operand' in err(lib)
    _operands(lib, call, p, ('weight', 'bias', 'q_hi', 'k_hi', 'v_hi', 'out_hi'))
    for k in ('q', 'k', 'v', 'out'):
        for q in ('q', 'k', 'v', 'out'):
            setattr(p, f'{q}_plane_stride', 16 * 24)
        setattr(p, f'{k}_plane_stride', 16 * 24 - 1)
        assert call() == E_ARG and b'plane stride' in err(lib), k
    p.out_plane_stride = 16 * 24
    H.each_misaligned(lib, call, p, ('q_hi', 'q_lo', 'k_hi', 'k_lo', 'v_hi', 'v_lo', 'out_hi', 'out_lo'), **ALIGN)


def test_spec_mul_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_spec_mul(None, None) == E_ARG and b'null params' in err(lib)
    p = LW.LawfftSpecMulParams()
    call = H.caller(lib.rsa_lawfft_spec_mul, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.scale = 2, 16, 13, 45, 1.0
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1)), E_ARG, b'geometry')
    p.C = 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in err(lib)
    p.C = 45
    assert call() == E_ARG and b'null operand' in err(lib)
    _operands(lib, call, p, ('a', 'b', 'out'))
    H.each_misaligned(lib, call, p, ('a', 'b', 'out'), **ALIGN)


def test_norm_mul_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_norm_mul(None, None) == E_ARG and b'null params' in err(lib)
    p = LW.LawfftNormMulParams()
    call = H.caller(lib.rsa_lawfft_norm_mul, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.eps = 1, 9, 11, 45, 1e-6
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1)), E_ARG, b'geometry')
    for key in ('fmt', 'corr_fmt'):
        setattr(p, key, 2)
        assert call() == E_ARG and b'plane format' in err(lib), key
        setattr(p, key, PF_BF16)
    p.C = 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in err(lib)
    p.C = 45
    assert call() == E_ARG and b'null operand' in err(lib)
    _operands(lib, call, p, ('weight', 'bias', 'corr_hi', 'v_hi', 'out_hi'))
    for k in ('corr', 'v', 'out'):
        for q in ('corr', 'v', 'out'):
            setattr(p, f'{q}_plane_stride', 99)
        setattr(p, f'{k}_plane_stride', 98)
        assert call() == E_ARG and b'plane stride' in err(lib), k
    p.out_plane_stride = 99
    H.each_misaligned(lib, call, p, ('corr_hi', 'corr_lo', 'v_hi', 'v_lo', 'out_hi', 'out_lo'), **ALIGN)


def test_kernel_gen_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_kernel_gen(None, None) == E_ARG and b'null params' in err(lib)
    p = LW.LawfftKernelGenParams()
    call = H.caller(lib.rsa_lawfft_kernel_gen, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.ksize = 3, 9, 11, 15, 3
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1), ('reserved1', 1)), E_ARG, b'geometry')
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in err(lib)
    p.fmt, p.C = PF_BF16, 129
    assert call() == E_UNSUPPORTED and b'C must be 1..128' in err(lib)
    p.C = 15
    H.each_bad(lib, call, p, [('ksize', k) for k in (0, 1, 4, 7)], E_UNSUPPORTED, b'ksize must be 3 or 5')
    p.ksize = 5
    assert call() == E_ARG and b'null operand' in err(lib)
    _operands(lib, call, p, ('w1_t', 'b1', 'w2_t', 'b2', 'workspace', 'out', 'in_hi'))
    p.in_plane_stride = 98
    assert call() == E_ARG and b'plane stride' in err(lib)
    p.in_plane_stride = 99
    H.each_misaligned(lib, call, p, ('in_hi', 'in_lo', 'workspace'), **ALIGN)


def test_kernel_gen_workspace_bytes():
    lib = L.load()
    q = lib.rsa_lawfft_kernel_gen_workspace_bytes
    assert q(1, 1, 8, 8) == 32 and q(3, 15, 8, 8) == 3 * 2 * 32 and q(2, 60, 24, 40) == 2 * 8 * 32  # one chunk of pixels up to 4096
    assert q(1, 8, 64, 65) == 2 * 32 and q(1, 128, 512, 512) == 16 * 64 * 32 and q(1, 8, 4096, 4096) == 64 * 32  # at most 64 chunks
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 129, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0)):
        assert q(*bad) == -1, bad


def test_dyn_dwconv_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_lawfft_dyn_dwconv(None, None) == E_ARG and b'null params' in err(lib)
    p = LW.LawfftDynDwConvParams()
    call = H.caller(lib.rsa_lawfft_dyn_dwconv, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.ksize = 2, 9, 11, 60, 3
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('reserved0', 1), ('reserved1', 1)), E_ARG, b'geometry')
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in err(lib)
    p.fmt = PF_BF16
    H.each_bad(lib, call, p, [('ksize', k) for k in (0, 1, 4, 7)], E_UNSUPPORTED, b'ksize must be 3 or 5')
    p.ksize = 3
    assert call() == E_ARG and b'null operand' in err(lib)
    _operands(lib, call, p, ('weight', 'in_hi', 'out_hi'))
    p.out_hi = None
    assert call() == E_ARG and b'null operand' in err(lib)  # neither planes nor an f32 map to write
    p.out_lo = 4096
    p.out_f32 = 8192
    assert call() == E_ARG and b'out_lo without out_hi' in err(lib)
    p.out_lo, p.out_hi = None, 3072
    p.in_plane_stride, p.out_plane_stride = 98, 99
    assert call() == E_ARG and b'plane stride' in err(lib)
    p.in_plane_stride, p.out_plane_stride = 99, 98
    assert call() == E_ARG and b'plane stride' in err(lib)
    p.out_plane_stride = 99
    keep, p.out_hi = p.out_hi, p.in_hi
    assert call() == E_ARG and b'not in place' in err(lib)
    p.out_hi = keep
    H.each_misaligned(lib, call, p, ('in_hi', 'in_lo', 'out_hi', 'out_lo', 'res1', 'res2', 'out_f32'), **ALIGN)


def test_pack_kernel_gen_transposes():
    c, k = 5, 3
    w1, b1 = torch.arange(c * c, dtype=torch.float32).reshape(c, c, 1, 1), torch.arange(c, dtype=torch.float32)
    w2, b2 = torch.arange(c * k * k * c, dtype=torch.float32).reshape(c * k * k, c, 1, 1), torch.arange(c * k * k, dtype=torch.float32)
    w1_t, b1_, w2_t, b2_ = LW.pack_kernel_gen(w1, b1, w2, b2)
    assert w1_t.shape == (c, c) and w2_t.shape == (c, c * k * k) and w1_t.is_contiguous() and w2_t.is_contiguous()
    assert w1_t[2, 4] == w1[4, 2, 0, 0] and w2_t[3, 17] == w2[17, 3, 0, 0] and torch.equal(b1_, b1) and torch.equal(b2_, b2)
    with pytest.raises(ValueError):
        LW.pack_kernel_gen(w1, b1, w2[:-1], b2[:-1])
