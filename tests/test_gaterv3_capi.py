"""The workspace sizes and the argument checks of every entry point of include/resselt_amd_gaterv3.h that need no GPU: each returns
before any launch.  tests/test_capi_headers.py compares the header with its ctypes mirrors, rows and chunk constants
(resselt_amd/engine/lib_gaterv3.py)."""

import capi_header as H
from capi_header import E_ARG, E_UNSUPPORTED, err
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gaterv3 as LG3


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


def _walk_pointers(lib, call, p, ptrs, optional=()):
    H.place(p, ptrs + tuple(optional), 4096)
    H.each_null(lib, call, p, ptrs, b'null pointer')


def test_local_gate_and_sca_apply_argument_validation_without_gpu():
    lib = L.load()
    for fn, cls, ptrs, planes, aligned in (
        (lib.rsa_gaterv3_local_gate, LG3.LocalGateParams, ('x_hi', 'weight', 'bias', 'out_hi', 'workspace'), ('x', 'out'), ('x_hi', 'x_lo', 'out_hi', 'out_lo', 'weight', 'bias', 'workspace')),
        (lib.rsa_gaterv3_sca_apply, LG3.ScaApplyParams, ('s_hi', 'sca_w', 'sca_b', 'gamma0', 'short_f32', 'out_f32', 'workspace'), ('s',),
         ('s_hi', 's_lo', 'sca_w', 'sca_b', 'gamma0', 'short_f32', 'out_f32', 'workspace')),
    ):  # fmt: skip
        assert fn(None, None) == E_ARG and b'null params' in err(lib)
        p = cls()
        call = H.caller(fn, p)
        assert call() == E_ARG and b'geometry' in err(lib)
        p.batch, p.H, p.W, p.dim, p.fmt = 2, 9, 33, 16, 1
        H.each_bad(lib, call, p, (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('dim', 0), ('fmt', 2), ('fmt', -1)), E_ARG, b'geometry')
        H.each_bad(lib, call, p, [('dim', dim) for dim in (4, 12, 520, 1024)], E_UNSUPPORTED, b'multiple of 8 up to 512')
        _walk_pointers(lib, call, p, ptrs, optional=tuple(f'{k}_lo' for k in planes))
        H.each_misaligned(lib, call, p, aligned, by=8)
        for k in planes:
            setattr(p, f'{k}_plane_stride', 9 * 33 - 1)
            assert call() == E_ARG and b'plane stride' in err(lib), k
            setattr(p, f'{k}_plane_stride', 9 * 33)
        need = lib.rsa_gaterv3_local_workspace_bytes(2, 9, 33, 16)
        if cls is LG3.LocalGateParams:
            keep = p.out_hi
            p.out_hi = p.x_hi
            assert call() == E_ARG and b'must not overlap' in err(lib)
            p.out_hi = keep
        p.workspace_bytes = need - 16
        assert call() == E_ARG and b'workspace too small' in err(lib)


def test_channel_attention_argument_validation_without_gpu():
    lib = L.load()
    fn = lib.rsa_gaterv3_channel_attention
    assert fn(None, None) == E_ARG and b'null params' in err(lib)
    p = LG3.AttnParams()
    call = H.caller(fn, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.heads, p.head_dim, p.fmt = 2, 5, 13, 32, 16, 2, 0
    H.each_bad(lib, call, p, (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('heads', 0), ('head_dim', 0), ('fmt', 2)), E_ARG, b'geometry')
    for c, heads, d in ((36, 16, 2), (32, 17, 2), (2080, 16, 65)):
        p.C, p.heads, p.head_dim = c, heads, d
        assert call() == E_UNSUPPORTED and b'heads 1..16, head_dim 1..64' in err(lib), (c, heads, d)
    p.C, p.heads, p.head_dim = 32, 16, 4
    assert call() == E_ARG and b'heads * head_dim must equal C' in err(lib)
    p.head_dim = 2
    _walk_pointers(lib, call, p, ('qkv_hi', 'temperature', 'out_hi', 'workspace'), optional=('qkv_lo', 'out_lo'))
    H.each_misaligned(lib, call, p, ('qkv_hi', 'qkv_lo', 'out_hi', 'out_lo', 'workspace'), by=8)
    for k in ('qkv', 'out'):
        setattr(p, f'{k}_plane_stride', 64)
        assert call() == E_ARG and b'plane stride' in err(lib), k
        setattr(p, f'{k}_plane_stride', 65)
    keep = p.out_hi
    p.out_hi = p.qkv_hi
    assert call() == E_ARG and b'must not overlap' in err(lib)
    p.out_hi = keep
    p.workspace_bytes = lib.rsa_gaterv3_attn_workspace_bytes(2, 5, 13, 16, 2) - 16
    assert call() == E_ARG and b'workspace too small' in err(lib)


def test_shortcut_argument_validation_without_gpu():
    lib = L.load()
    fn = lib.rsa_gaterv3_shortcut
    assert fn(None, None) == E_ARG and b'null params' in err(lib)
    p = LG3.ShortcutParams()
    call = H.caller(fn, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.C, p.h, p.w, p.scale, p.out_H, p.out_W, p.dtype = 2, 3, 5, 7, 3, 24, 24, 0
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('C', 0), ('h', 0), ('w', 0), ('scale', 0), ('scale', 9)), E_ARG, b'geometry')
    H.each_bad(lib, call, p, (('out_H', 14), ('out_W', 20)), E_ARG, b'smaller than the scaled input')
    _walk_pointers(lib, call, p, ('x', 'gamma', 'out'))
    for dtype in (3, 4, -1):
        p.dtype = dtype
        assert call() == E_UNSUPPORTED and b'dtype must be f32, f16 or bf16' in err(lib), dtype
