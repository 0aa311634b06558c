"""include/resselt_amd_figsr.h against its ctypes mirrors and signature rows (resselt_amd/engine/lib_figsr.py): the same structs with the
same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, the argument checks that need no GPU, and the band weight packer against a plain-numpy statement of the layout the header
gives.  The parsers are those of tests/test_moesr_capi.py, pointed at this header."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import test_moesr_capi as P
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_figsr as LF
from resselt_amd.engine import lib_gfisr as LG
from resselt_amd.engine.tensors import PF_BF16, PF_F16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_figsr.h')
MIRRORS = {'rsa_figsr_mix_params': LF.FigsrMixParams, 'rsa_figsr_input_params': LF.FigsrInputParams, 'rsa_figsr_output_params': LF.FigsrOutputParams}
ENTRIES = ['rsa_figsr_mix', 'rsa_figsr_band_packed_weight_bytes', 'rsa_figsr_input', 'rsa_figsr_output']
SIZES = {'rsa_figsr_mix_params': 10 * 4 + 3 * 8 + 4 * 4 * 8, 'rsa_figsr_input_params': 8 * 4 + 3 * 8 + 4 * 8, 'rsa_figsr_output_params': 10 * 4 + 4 * 8}
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
    assert list(protos) == list(LF.SIGNATURES) == ENTRIES
    names = {ctypes.POINTER(m): n for n, m in MIRRORS.items()}
    names.update({ctypes.c_void_p: 'ptr', ctypes.c_int32: 'int32_t'})
    rets = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t'}
    for entry, (restype, params) in LF.SIGNATURES.items():
        assert rets[restype] == protos[entry][0], entry
        assert [(k, names[t]) for k, t in params] == protos[entry][1], entry


def test_the_main_tables_do_not_know_them_and_the_library_does():
    for entry, row in LF.SIGNATURES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS and L.EXTENSIONS[entry] is row and L.signature(entry) is row
        assert entry not in LG.SIGNATURES  # the GFISR header keeps its four names
    assert list(LG.SIGNATURES) == ['rsa_gfisr_dft', 'rsa_gfisr_dft_scratch_bytes', 'rsa_gfisr_spectral', 'rsa_gfisr_gate']
    assert '#include "resselt_amd.h"' in open(HEADER).read()
    for other in ('resselt_amd.h', 'resselt_amd_gfisr.h'):
        assert 'figsr' not in open(os.path.join(ROOT, 'include', other)).read()
    lib = L.load()
    for entry, (restype, params) in LF.SIGNATURES.items():
        fn = getattr(lib, entry)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params]


def _err(lib):
    return lib.rsa_last_error_string()


def test_mix_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_figsr_mix(None, None) == E_ARG and b'null params' in _err(lib)
    p = LF.FigsrMixParams()
    call = lambda: lib.rsa_figsr_mix(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.H, p.W, p.fmt, p.products, p.ksize, p.gc, p.planes, p.pass_planes = 1, 4, 6, PF_BF16, 3, 17, 8, 8, 5
    for key, bad in (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('reserved0', 1)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert call() == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in _err(lib)
    p.fmt, p.products = PF_BF16, 2
    assert call() == E_ARG and b'products must be 1 or 3' in _err(lib)
    p.products = 3
    for k in (1, 4, 16, 33):
        p.ksize = k
        assert call() == E_UNSUPPORTED and b'ksize must be odd, 3..31' in _err(lib), k
    p.ksize = 17
    for gc in (0, 4, 12, 24):
        p.gc = gc
        assert call() == E_UNSUPPORTED and b'gc must be 8 or 16' in _err(lib), gc
    p.gc = 8
    for planes, pas in ((7, 5), (9, 5), (2, -1)):
        p.planes, p.pass_planes = planes, pas
        assert call() == E_ARG and b'pass_planes + 3 gc / 8' in _err(lib)
    p.planes, p.pass_planes = 8, 5
    assert call() == E_ARG and b'null operand' in _err(lib)
    ptrs = ('w_packed', 'bias_w', 'bias_h', 'g_hi', 'x_hi', 'hw_hi', 'out_hi')
    for i, k in enumerate(ptrs):
        setattr(p, k, 1024 * (i + 1))
    p.x_lo = 1 << 20
    for k in ptrs:
        keep = getattr(p, k)
        setattr(p, k, None)
        assert call() == E_ARG and b'null operand' in _err(lib), k
        setattr(p, k, keep)
    p.x_lo = None
    assert call() == E_ARG and b'three products need x_lo' in _err(lib)
    p.x_lo = 1 << 20
    for k in ('g', 'x', 'hw', 'out'):
        for q in ('g', 'x', 'hw', 'out'):
            setattr(p, f'{q}_plane_stride', 24)
        setattr(p, f'{k}_plane_stride', 23)
        assert call() == E_ARG and b'plane stride' in _err(lib), k
    p.out_plane_stride = 24
    for k in ('g_hi', 'x_hi', 'hw_hi'):
        keep, p.out_hi = p.out_hi, getattr(p, k)
        assert call() == E_ARG and b'out must not be' in _err(lib), k
        p.out_hi = keep
    for k in ptrs + ('g_lo', 'x_lo', 'hw_lo', 'out_lo'):
        keep = getattr(p, k)
        setattr(p, k, (1 << 21) + 8)
        assert call() == E_ALIGN and b'16-byte aligned' in _err(lib), k
        setattr(p, k, keep)
    # the two compiled pairs are (bf16, 3 products) and (fp16, 1 product): the others are refused by name
    p.products = 1
    assert call() == E_UNSUPPORTED and b'compiled for bf16 planes with three products' in _err(lib)
    p.fmt, p.products = PF_F16, 3
    assert call() == E_UNSUPPORTED and b'compiled for bf16 planes with three products' in _err(lib)


def test_band_packed_weight_bytes():
    lib = L.load()
    for k in (3, 11, 17, 31):
        for gc in (8, 16):
            for products in (1, 3):
                want = 2 * (gc // 8) * ((k + 3) // 4) * (2 if products == 3 else 1) * 64 * 16
                assert lib.rsa_figsr_band_packed_weight_bytes(k, gc, products) == want
    for bad in ((1, 8, 3), (4, 8, 3), (33, 8, 3), (17, 4, 3), (17, 24, 3), (17, 8, 2), (17, 8, 0)):
        assert lib.rsa_figsr_band_packed_weight_bytes(*bad) == -1, bad


def test_input_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_figsr_input(None, None) == E_ARG and b'null params' in _err(lib)
    p = LF.FigsrInputParams()
    call = lambda: lib.rsa_figsr_input(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.C, p.src_h, p.src_w, p.pad = 1, 3, 6, 7, 4
    for key, bad in (('batch', 0), ('C', 0), ('src_h', 0), ('src_w', 0), ('reserved0', 1)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert call() == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    p.C = 9
    assert call() == E_UNSUPPORTED and b'at most 8 channels' in _err(lib)
    p.C = 3
    for h, w, pad in ((5, 6, 4), (6, 5, 4), (4, 8, 4), (8, 4, 4), (6, 6, -1)):  # 4 + size % 2 must stay below the size
        p.src_h, p.src_w, p.pad = h, w, pad
        assert call() == E_ARG and b'the reflection needs' in _err(lib), (h, w, pad)
    p.src_h, p.src_w, p.pad, p.dtype = 6, 7, 4, L.U8
    assert call() == E_ARG and b'bad dtype' in _err(lib)
    p.dtype, p.fmt = L.F32, 2
    assert call() == E_ARG and b'plane format' in _err(lib)
    p.fmt = PF_BF16
    ptrs = ('x', 'shift', 'scale_norm', 'out_hi')
    for k in ptrs:
        setattr(p, k, 64)
    for k in ptrs:
        setattr(p, k, None)
        assert call() == E_ARG and b'null operand' in _err(lib), k
        setattr(p, k, 64)
    for k in ('out_hi', 'out_lo'):
        keep = getattr(p, k)
        setattr(p, k, 72)
        assert call() == E_ALIGN and b'16-byte aligned' in _err(lib), k
        setattr(p, k, keep)
    p.out_plane_stride = 14 * 16 - 1  # 6 x 7 pads to 14 x 16
    assert call() == E_ARG and b'plane stride' in _err(lib)


def test_output_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_figsr_output(None, None) == E_ARG and b'null params' in _err(lib)
    p = LF.FigsrOutputParams()
    call = lambda: lib.rsa_figsr_output(ctypes.byref(p), None)  # noqa: E731
    assert call() == E_ARG and b'geometry' in _err(lib)
    p.batch, p.C, p.H, p.W, p.y0, p.x0, p.out_h, p.out_w = 1, 3, 28, 32, 8, 8, 12, 14
    for key, bad in (('batch', 0), ('C', 0), ('H', 0), ('W', 0), ('out_h', 0), ('out_w', 0), ('reserved0', 1)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert call() == E_ARG and b'geometry' in _err(lib), key
        setattr(p, key, keep)
    for key, bad in (('y0', -1), ('x0', -1), ('y0', 17), ('x0', 19), ('out_h', 21), ('out_w', 25)):
        keep = getattr(p, key)
        setattr(p, key, bad)
        assert call() == E_ARG and b'window leaves the map' in _err(lib), key
        setattr(p, key, keep)
    p.dtype = L.U8
    assert call() == E_ARG and b'bad dtype' in _err(lib)
    p.dtype = L.F16
    ptrs = ('y', 'shift', 'scale_norm', 'out')
    for k in ptrs:
        setattr(p, k, 64)
    for k in ptrs:
        setattr(p, k, None)
        assert call() == E_ARG and b'null operand' in _err(lib), k
        setattr(p, k, 64)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.view(torch.int16).numpy().astype(np.uint16)


@pytest.mark.parametrize('k,gc,products,fmt', [(3, 8, 3, PF_BF16), (17, 8, 3, PF_BF16), (11, 16, 3, PF_BF16), (31, 16, 1, PF_F16), (5, 8, 1, PF_F16)])
def test_band_packer_matches_the_layout_the_header_gives(k, gc, products, fmt):
    """blob[band][p][s][half][lane][j] = W_band[lane & 15][8 p + j][tap 4 s + (lane >> 4)], zero past K and past output channel gc;
    half 0 the value rounded to the format, half 1 (three products) the rounded residual."""
    gen = torch.Generator().manual_seed(100 * k + gc)
    w_w, w_h = torch.randn(gc, gc, 1, k, generator=gen), torch.randn(gc, gc, k, 1, generator=gen)
    blob = LF.pack_band_weights(w_w, w_h, products, fmt)
    P_, S, HL = gc // 8, (k + 3) // 4, 2 if products == 3 else 1
    assert blob.dtype == torch.bfloat16 and blob.numel() * 2 == L.load().rsa_figsr_band_packed_weight_bytes(k, gc, products)
    got = _bits(blob).reshape(2, P_, S, HL, 64, 8)
    dt = torch.float16 if fmt == PF_F16 else torch.bfloat16
    taps = [w_w.reshape(gc, gc, k).numpy(), w_h.reshape(gc, gc, k).numpy()]
    want = np.zeros((2, P_, S, HL, 64, 8), dtype=np.float32)
    for band in range(2):
        for p in range(P_):
            for s in range(S):
                for lane in range(64):
                    co, t = lane & 15, 4 * s + (lane >> 4)
                    if co < gc and t < k:
                        want[band, p, s, :, lane, :] = taps[band][co, 8 * p : 8 * p + 8, t]
    full = torch.from_numpy(want[:, :, :, 0])
    hi = full.to(dt)
    assert np.array_equal(got[:, :, :, 0], _bits(hi))
    if products == 3:
        assert np.array_equal(got[:, :, :, 1], _bits((full - hi.float()).to(dt)))
    with pytest.raises(ValueError):
        LF.pack_band_weights(w_w, w_w, products, fmt)
    assert torch.equal(LF.band_bias(torch.arange(gc, dtype=torch.float32))[:gc], torch.arange(gc, dtype=torch.float32)) and LF.band_bias(torch.ones(gc)).numel() == 16
