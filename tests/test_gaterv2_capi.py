"""The workspace sizes and the argument checks of ``rsa_gaterv2_linear_attention`` (include/resselt_amd_gaterv2.h) that need no GPU: each
returns before any launch.  tests/test_capi_headers.py compares the header with its ctypes mirror, rows and chunk constant
(resselt_amd/engine/lib_gaterv2.py).  Also here, because it needs no GPU: the conditioning of every input the GPU kernel test builds
(tests/test_gaterv2_kernels_gpu.py asserts it again on the values the kernel reads)."""

import torch

import capi_header as H
from capi_header import E_ARG, E_UNSUPPORTED, err
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gaterv2 as LG2


def test_workspace_sizes():
    lib = L.load()
    for n, h, w, c, m in ((1, 1, 1, 16, 1), (2, 5, 13, 32, 2), (3, 8, 16, 96, 6), (2, 3, 43, 768, 48), (1, 32, 32, 768, 48), (1, 15, 20, 1024, 64), (2, 4, 4, 16, 16)):
        chunks = -(-h * w // LG2.TOKEN_CHUNK)
        assert lib.rsa_gaterv2_attn_workspace_bytes(n, h, w, c, m) == (4 * n * (chunks + 1) * LG2.record_floats(c, m) + 15) // 16 * 16
    for bad in ((0, 4, 4, 16, 1), (65536, 4, 4, 16, 1), (1, 0, 4, 16, 1), (1, 4, 0, 16, 1), (1, 4, 4, 0, 1), (1, 4, 4, 8, 1), (1, 4, 4, 20, 1), (1, 4, 4, 1032, 64),
                (1, 4, 4, 16, 0), (1, 4, 4, 128, 65), (1, 4, 4, 16, 17)):  # fmt: skip
        assert lib.rsa_gaterv2_attn_workspace_bytes(*bad) <= 0, bad


def test_linear_attention_argument_validation_without_gpu():
    lib = L.load()
    fn = lib.rsa_gaterv2_linear_attention
    assert fn(None, None) == E_ARG and b'null params' in err(lib)
    p = LG2.AttnParams()
    call = H.caller(fn, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.m, p.fmt, p.eps = 2, 5, 13, 32, 2, 0, 1e-6
    H.each_bad(lib, call, p, (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('m', 0), ('fmt', 2), ('fmt', -1)), E_ARG, b'geometry')
    for c, m in ((8, 1), (36, 2), (1032, 2), (2048, 64), (128, 65)):
        p.C, p.m = c, m
        assert call() == E_UNSUPPORTED and b'multiple of 8 in 16..1024, m 1..64' in err(lib), (c, m)
    p.C, p.m = 16, 17
    assert call() == E_ARG and b'm must not exceed C' in err(lib)
    p.C, p.m = 32, 2
    ptrs, optional = ('qkv_hi', 'out_hi', 'workspace'), ('qkv_lo', 'out_lo')
    H.place(p, ptrs + optional, 4096)
    H.each_null(lib, call, p, ptrs, b'null pointer')
    H.each_misaligned(lib, call, p, ('qkv_hi', 'qkv_lo', 'out_hi', 'out_lo', 'workspace'), by=8)
    for k in ('qkv', 'out'):
        setattr(p, f'{k}_plane_stride', 64)
        assert call() == E_ARG and b'plane stride' in err(lib), k
        setattr(p, f'{k}_plane_stride', 65)
    for k in ('qkv', 'out'):
        setattr(p, f'{k}_batch_stride', -1)
        assert call() == E_ARG and b'plane stride' in err(lib), k
        setattr(p, f'{k}_batch_stride', 6 * 65)
    keep = p.out_hi
    p.out_hi = p.qkv_hi
    assert call() == E_ARG and b'must not overlap' in err(lib)
    p.out_hi = keep
    keep = p.out_lo
    p.out_lo = p.qkv_lo
    assert call() == E_ARG and b'must not overlap' in err(lib)
    p.out_lo = keep
    p.workspace_bytes = lib.rsa_gaterv2_attn_workspace_bytes(2, 5, 13, 32, 2) - 16
    assert call() == E_ARG and b'workspace too small' in err(lib)


def test_the_gpu_kernel_tests_inputs_are_well_conditioned():
    """Every case of tests/test_gaterv2_kernels_gpu.py, on the values the kernel reads in each plane format: its reference asserts that every
    q and k token vector has a norm of at least 0.25 and that the denominator is at least N / 2."""
    import gaterv2_attn_cases as K
    from resselt_amd.engine.tensors import nchw_to_planes, planes_to_nchw

    for c, m, hw in K.CASES:
        x = K.make_inputs(c, m, hw)
        for fmt, with_lo in K.FORMATS:
            read = planes_to_nchw(nchw_to_planes(x, with_lo, fmt), x.shape[1]).double()
            ref, bar = K.reference(read, c, m, fmt, with_lo)
            assert ref.shape == (3, c, *hw) and bool(torch.isfinite(ref).all()) and bool((bar > 0).all())
