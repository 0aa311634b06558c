"""include/resselt_amd_gaterv2.h against its ctypes mirror and signature rows (resselt_amd/engine/lib_gaterv2.py): the same struct with the
same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, the chunk constant, the workspace sizes and the argument checks that need no GPU.  The parsers are those of
tests/test_moesr_capi.py, pointed at this header.  Also here, because it needs no GPU: the conditioning of every input the GPU kernel test
builds (tests/test_gaterv2_kernels_gpu.py asserts it again on the values the kernel reads)."""

import ctypes
import os
import re

import pytest
import torch

import test_moesr_capi as P
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gaterv2 as LG2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_gaterv2.h')
MIRRORS = {'rsa_gaterv2_attn_params': LG2.AttnParams}
E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3


@pytest.fixture
def header(monkeypatch):
    text = open(HEADER).read()
    monkeypatch.setattr(P, '_header', lambda: re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))


def test_the_struct_matches_its_mirror(header):
    structs = P._header_structs()
    assert list(structs) == list(MIRRORS)
    classes = {ctypes.c_int32: 'int32_t', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float', ctypes.c_void_p: 'pointer'}
    for name, mirror in MIRRORS.items():
        assert name in mirror.__doc__
        assert [(k, classes[t]) for k, t in mirror._fields_] == structs[name]
    assert [k for k, _ in LG2.AttnParams._fields_][:8] == ['batch', 'H', 'W', 'C', 'm', 'fmt', 'eps', 'reserved0']
    assert ctypes.sizeof(LG2.AttnParams) == 8 * 4 + 32 + 32 + 2 * 8  # no padding: the C compiler lays it out the same way


def test_the_prototypes_match_their_rows(header):
    protos = P._header_prototypes()
    assert list(protos) == list(LG2.SIGNATURES)
    names = {ctypes.POINTER(m): n for n, m in MIRRORS.items()}
    names.update({ctypes.c_void_p: 'ptr', ctypes.c_int32: 'int32_t'})
    for entry, (restype, params) in LG2.SIGNATURES.items():
        assert {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t'}[restype] == protos[entry][0], entry
        assert [(k, names[t]) for k, t in params] == protos[entry][1], entry


def test_the_chunk_constant_matches_the_header():
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r'#define\s+RSA_GATERV2_(\w+)\s+(\d+)', text)}
    assert consts == {'TOKEN_CHUNK': LG2.TOKEN_CHUNK}


def test_the_main_tables_do_not_know_them_and_the_library_does():
    for entry, row in LG2.SIGNATURES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS
        assert L.EXTENSIONS[entry] is row and L.signature(entry) is row
    assert '#include "resselt_amd.h"' in open(HEADER).read()
    lib = L.load()
    for entry, (restype, params) in LG2.SIGNATURES.items():
        fn = getattr(lib, entry)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params]


def test_workspace_sizes():
    lib = L.load()
    for n, h, w, c, m in ((1, 1, 1, 16, 1), (2, 5, 13, 32, 2), (3, 8, 16, 96, 6), (2, 3, 43, 768, 48), (1, 32, 32, 768, 48), (1, 15, 20, 1024, 64), (2, 4, 4, 16, 16)):
        chunks = -(-h * w // LG2.TOKEN_CHUNK)
        assert lib.rsa_gaterv2_attn_workspace_bytes(n, h, w, c, m) == (4 * n * (chunks + 1) * LG2.record_floats(c, m) + 15) // 16 * 16
    for bad in ((0, 4, 4, 16, 1), (65536, 4, 4, 16, 1), (1, 0, 4, 16, 1), (1, 4, 0, 16, 1), (1, 4, 4, 0, 1), (1, 4, 4, 8, 1), (1, 4, 4, 20, 1), (1, 4, 4, 1032, 64),
                (1, 4, 4, 16, 0), (1, 4, 4, 128, 65), (1, 4, 4, 16, 17)):  # fmt: skip
        assert lib.rsa_gaterv2_attn_workspace_bytes(*bad) <= 0, bad


def _err(lib):
    return lib.rsa_last_error_string()


def test_linear_attention_argument_validation_without_gpu():
    lib = L.load()
    fn = lib.rsa_gaterv2_linear_attention
    assert fn(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG2.AttnParams()
    assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.m, p.fmt, p.eps = 2, 5, 13, 32, 2, 0, 1e-6
    for key, bad in (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('m', 0), ('fmt', 2), ('fmt', -1)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    for c, m in ((8, 1), (36, 2), (1032, 2), (2048, 64), (128, 65)):
        p.C, p.m = c, m
        assert fn(ctypes.byref(p), None) == E_UNSUPPORTED and b'multiple of 8 in 16..1024, m 1..64' in _err(lib), (c, m)
    p.C, p.m = 16, 17
    assert fn(ctypes.byref(p), None) == E_ARG and b'm must not exceed C' in _err(lib)
    p.C, p.m = 32, 2
    ptrs, optional = ('qkv_hi', 'out_hi', 'workspace'), ('qkv_lo', 'out_lo')
    for i, k in enumerate(ptrs + optional):
        setattr(p, k, 4096 * (i + 1))
    for i, k in enumerate(ptrs):
        setattr(p, k, None)
        assert fn(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib), k
        setattr(p, k, 4096 * (i + 1))
    for k in ('qkv_hi', 'qkv_lo', 'out_hi', 'out_lo', 'workspace'):
        keep = getattr(p, k)
        setattr(p, k, keep + 8)
        assert fn(ctypes.byref(p), None) == E_ALIGN, k
        setattr(p, k, keep)
    for k in ('qkv', 'out'):
        setattr(p, f'{k}_plane_stride', 64)
        assert fn(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib), k
        setattr(p, f'{k}_plane_stride', 65)
    for k in ('qkv', 'out'):
        setattr(p, f'{k}_batch_stride', -1)
        assert fn(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib), k
        setattr(p, f'{k}_batch_stride', 6 * 65)
    keep = p.out_hi
    p.out_hi = p.qkv_hi
    assert fn(ctypes.byref(p), None) == E_ARG and b'must not overlap' in _err(lib)
    p.out_hi = keep
    keep = p.out_lo
    p.out_lo = p.qkv_lo
    assert fn(ctypes.byref(p), None) == E_ARG and b'must not overlap' in _err(lib)
    p.out_lo = keep
    p.workspace_bytes = lib.rsa_gaterv2_attn_workspace_bytes(2, 5, 13, 32, 2) - 16
    assert fn(ctypes.byref(p), None) == E_ARG and b'workspace too small' in _err(lib)


def test_the_gpu_kernel_tests_inputs_are_well_conditioned():
    """Every case of tests/test_gaterv2_kernels_gpu.py, on the values the kernel reads in each plane format: its reference asserts that every
    q and k token vector has a norm of at least 0.25 and that the denominator is at least N / 2."""
    import test_gaterv2_kernels_gpu as K
    from resselt_amd.engine.tensors import nchw_to_planes, planes_to_nchw

    for c, m, hw in K.CASES:
        x = K.make_inputs(c, m, hw)
        for fmt, with_lo in K.FORMATS:
            read = planes_to_nchw(nchw_to_planes(x, with_lo, fmt), x.shape[1]).double()
            ref, bar = K.reference(read, c, m, fmt, with_lo)
            assert ref.shape == (3, c, *hw) and bool(torch.isfinite(ref).all()) and bool((bar > 0).all())
