"""include/resselt_amd_gaterv3.h against its ctypes mirrors and signature rows (resselt_amd/engine/lib_gaterv3.py): the same structs with the
same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, the chunk constants, the workspace sizes and the argument checks that need no GPU.  The parsers are those of
tests/test_moesr_capi.py, pointed at this header."""

import ctypes
import os
import re

import pytest

import test_moesr_capi as P
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gaterv3 as LG3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_gaterv3.h')
MIRRORS = {'rsa_gaterv3_local_gate_params': LG3.LocalGateParams, 'rsa_gaterv3_sca_apply_params': LG3.ScaApplyParams,
           'rsa_gaterv3_attn_params': LG3.AttnParams, 'rsa_gaterv3_shortcut_params': LG3.ShortcutParams}  # fmt: skip
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
    # no padding: the C compiler lays them out the same way
    assert ctypes.sizeof(LG3.LocalGateParams) == 6 * 4 + 32 + 2 * 8 + 32 + 2 * 8
    assert ctypes.sizeof(LG3.ScaApplyParams) == 6 * 4 + 32 + 5 * 8 + 2 * 8
    assert ctypes.sizeof(LG3.AttnParams) == 8 * 4 + 32 + 8 + 32 + 2 * 8
    assert ctypes.sizeof(LG3.ShortcutParams) == 8 * 4 + 3 * 8


def test_the_prototypes_match_their_rows(header):
    protos = P._header_prototypes()
    assert list(protos) == list(LG3.SIGNATURES)
    names = {ctypes.POINTER(m): n for n, m in MIRRORS.items()}
    names.update({ctypes.c_void_p: 'ptr', ctypes.c_int32: 'int32_t'})
    for entry, (restype, params) in LG3.SIGNATURES.items():
        assert {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t'}[restype] == protos[entry][0], entry
        assert [(k, names[t]) for k, t in params] == protos[entry][1], entry


def test_the_chunk_constants_match_the_header():
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r'#define\s+RSA_GATERV3_(\w+)\s+(\d+)', text)}
    assert consts == {'TILE_W': LG3.TILE_W, 'TILE_H': LG3.TILE_H, 'TOKEN_CHUNK': LG3.TOKEN_CHUNK}


def test_the_main_tables_do_not_know_them_and_the_library_does():
    for entry, row in LG3.SIGNATURES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS
        assert L.EXTENSIONS[entry] is row and L.signature(entry) is row
    assert '#include "resselt_amd.h"' in open(HEADER).read()
    lib = L.load()
    for entry, (restype, params) in LG3.SIGNATURES.items():
        fn = getattr(lib, entry)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params]


def test_workspace_sizes():
    lib = L.load()
    tiles = lambda h, w: -(-h // LG3.TILE_H) * -(-w // LG3.TILE_W)  # noqa: E731
    for n, h, w, dim in ((1, 1, 1, 8), (2, 8, 32, 16), (2, 9, 33, 32), (3, 64, 25, 128), (1, 512, 512, 512)):
        assert lib.rsa_gaterv3_local_workspace_bytes(n, h, w, dim) == (4 * n * (tiles(h, w) + 1) * dim + 15) // 16 * 16
    for bad in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (1, 4, 4, 12), (1, 4, 4, 520), (65536, 4, 4, 8)):
        assert lib.rsa_gaterv3_local_workspace_bytes(*bad) <= 0, bad
    for n, h, w, heads, d in ((1, 1, 1, 16, 1), (2, 5, 13, 16, 2), (2, 13, 79, 16, 64), (1, 16, 8, 4, 6)):
        chunks = -(-h * w // LG3.TOKEN_CHUNK)
        assert lib.rsa_gaterv3_attn_workspace_bytes(n, h, w, heads, d) == (4 * n * heads * (chunks * (d * d + 2 * d) + d * d) + 15) // 16 * 16
    for bad in ((0, 4, 4, 16, 4), (1, 0, 4, 16, 4), (1, 4, 4, 0, 4), (1, 4, 4, 17, 4), (1, 4, 4, 16, 0), (1, 4, 4, 16, 65)):
        assert lib.rsa_gaterv3_attn_workspace_bytes(*bad) <= 0, bad


def _err(lib):
    return lib.rsa_last_error_string()


def _walk_pointers(lib, fn, p, ptrs, optional=()):
    for i, k in enumerate(ptrs + tuple(optional)):
        setattr(p, k, 4096 * (i + 1))
    for i, k in enumerate(ptrs):
        setattr(p, k, None)
        assert fn(ctypes.byref(p), None) == E_ARG and b'null pointer' in _err(lib), k
        setattr(p, k, 4096 * (i + 1))


def test_local_gate_and_sca_apply_argument_validation_without_gpu():
    lib = L.load()
    for fn, cls, ptrs, planes, aligned in (
        (lib.rsa_gaterv3_local_gate, LG3.LocalGateParams, ('x_hi', 'weight', 'bias', 'out_hi', 'workspace'), ('x', 'out'), ('x_hi', 'x_lo', 'out_hi', 'out_lo', 'weight', 'bias', 'workspace')),
        (lib.rsa_gaterv3_sca_apply, LG3.ScaApplyParams, ('s_hi', 'sca_w', 'sca_b', 'gamma0', 'short_f32', 'out_f32', 'workspace'), ('s',),
         ('s_hi', 's_lo', 'sca_w', 'sca_b', 'gamma0', 'short_f32', 'out_f32', 'workspace')),
    ):  # fmt: skip
        assert fn(None, None) == E_ARG and b'null params' in _err(lib)
        p = cls()
        assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
        p.batch, p.H, p.W, p.dim, p.fmt = 2, 9, 33, 16, 1
        for key, bad in (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('dim', 0), ('fmt', 2), ('fmt', -1)):
            keep = getattr(p, key)
            setattr(p, key, bad)
            assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
            setattr(p, key, keep)
        for dim in (4, 12, 520, 1024):
            p.dim = dim
            assert fn(ctypes.byref(p), None) == E_UNSUPPORTED and b'multiple of 8 up to 512' in _err(lib), dim
        p.dim = 16
        _walk_pointers(lib, fn, p, ptrs, optional=tuple(f'{k}_lo' for k in planes))
        for k in aligned:
            keep = getattr(p, k)
            setattr(p, k, keep + 8)
            assert fn(ctypes.byref(p), None) == E_ALIGN, k
            setattr(p, k, keep)
        for k in planes:
            setattr(p, f'{k}_plane_stride', 9 * 33 - 1)
            assert fn(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib), k
            setattr(p, f'{k}_plane_stride', 9 * 33)
        need = lib.rsa_gaterv3_local_workspace_bytes(2, 9, 33, 16)
        if cls is LG3.LocalGateParams:
            keep = p.out_hi
            p.out_hi = p.x_hi
            assert fn(ctypes.byref(p), None) == E_ARG and b'must not overlap' in _err(lib)
            p.out_hi = keep
        p.workspace_bytes = need - 16
        assert fn(ctypes.byref(p), None) == E_ARG and b'workspace too small' in _err(lib)


def test_channel_attention_argument_validation_without_gpu():
    lib = L.load()
    fn = lib.rsa_gaterv3_channel_attention
    assert fn(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG3.AttnParams()
    assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.C, p.heads, p.head_dim, p.fmt = 2, 5, 13, 32, 16, 2, 0
    for key, bad in (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('heads', 0), ('head_dim', 0), ('fmt', 2)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    for c, heads, d in ((36, 16, 2), (32, 17, 2), (2080, 16, 65)):
        p.C, p.heads, p.head_dim = c, heads, d
        assert fn(ctypes.byref(p), None) == E_UNSUPPORTED and b'heads 1..16, head_dim 1..64' in _err(lib), (c, heads, d)
    p.C, p.heads, p.head_dim = 32, 16, 4
    assert fn(ctypes.byref(p), None) == E_ARG and b'heads * head_dim must equal C' in _err(lib)
    p.head_dim = 2
    _walk_pointers(lib, fn, p, ('qkv_hi', 'temperature', 'out_hi', 'workspace'), optional=('qkv_lo', 'out_lo'))
    for k in ('qkv_hi', 'qkv_lo', 'out_hi', 'out_lo', 'workspace'):
        keep = getattr(p, k)
        setattr(p, k, keep + 8)
        assert fn(ctypes.byref(p), None) == E_ALIGN, k
        setattr(p, k, keep)
    for k in ('qkv', 'out'):
        setattr(p, f'{k}_plane_stride', 64)
        assert fn(ctypes.byref(p), None) == E_ARG and b'plane stride' in _err(lib), k
        setattr(p, f'{k}_plane_stride', 65)
    keep = p.out_hi
    p.out_hi = p.qkv_hi
    assert fn(ctypes.byref(p), None) == E_ARG and b'must not overlap' in _err(lib)
    p.out_hi = keep
    p.workspace_bytes = lib.rsa_gaterv3_attn_workspace_bytes(2, 5, 13, 16, 2) - 16
    assert fn(ctypes.byref(p), None) == E_ARG and b'workspace too small' in _err(lib)


def test_shortcut_argument_validation_without_gpu():
    lib = L.load()
    fn = lib.rsa_gaterv3_shortcut
    assert fn(None, None) == E_ARG and b'null params' in _err(lib)
    p = LG3.ShortcutParams()
    assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib)
    p.batch, p.C, p.h, p.w, p.scale, p.out_H, p.out_W, p.dtype = 2, 3, 5, 7, 3, 24, 24, 0
    for key, bad in (('batch', 0), ('batch', 65536), ('C', 0), ('h', 0), ('w', 0), ('scale', 0), ('scale', 9)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert fn(ctypes.byref(p), None) == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    for key, bad in (('out_H', 14), ('out_W', 20)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert fn(ctypes.byref(p), None) == E_ARG and b'smaller than the scaled input' in _err(lib), key
        setattr(p, key, keep)
    _walk_pointers(lib, fn, p, ('x', 'gamma', 'out'))
    for dtype in (3, 4, -1):
        p.dtype = dtype
        assert fn(ctypes.byref(p), None) == E_UNSUPPORTED and b'dtype must be f32, f16 or bf16' in _err(lib), dtype
