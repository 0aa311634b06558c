"""The argument checks of ``rsa_figsr_mix``, ``rsa_figsr_input`` and ``rsa_figsr_output`` (include/resselt_amd_figsr.h) that need no GPU
(each returns before any launch), the packed size, and the band weight packer against a plain-numpy statement of the layout the header
gives.  tests/test_capi_headers.py compares the header with its ctypes mirrors and rows (resselt_amd/engine/lib_figsr.py)."""

import numpy as np
import pytest
import torch

import capi_header as H
from capi_header import E_ALIGN, E_ARG, E_UNSUPPORTED, err
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_figsr as LF
from resselt_amd.engine.tensors import PF_BF16, PF_F16


def test_mix_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_figsr_mix(None, None) == E_ARG and b'null params' in err(lib)
    p = LF.FigsrMixParams()
    call = H.caller(lib.rsa_figsr_mix, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.fmt, p.products, p.ksize, p.gc, p.planes, p.pass_planes = 1, 4, 6, PF_BF16, 3, 17, 8, 8, 5
    H.each_bad(lib, call, p, (('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('reserved0', 1)), E_ARG, b'geometry')
    p.fmt = 2
    assert call() == E_ARG and b'plane format' in err(lib)
    p.fmt, p.products = PF_BF16, 2
    assert call() == E_ARG and b'products must be 1 or 3' in err(lib)
    p.products = 3
    H.each_bad(lib, call, p, [('ksize', k) for k in (1, 4, 16, 33)], E_UNSUPPORTED, b'ksize must be odd, 3..31')
    H.each_bad(lib, call, p, [('gc', gc) for gc in (0, 4, 12, 24)], E_UNSUPPORTED, b'gc must be 8 or 16')
    for planes, pas in ((7, 5), (9, 5), (2, -1)):
        p.planes, p.pass_planes = planes, pas
        assert call() == E_ARG and b'pass_planes + 3 gc / 8' in err(lib)
    p.planes, p.pass_planes = 8, 5
    assert call() == E_ARG and b'null operand' in err(lib)
    ptrs = ('w_packed', 'bias_w', 'bias_h', 'g_hi', 'x_hi', 'hw_hi', 'out_hi')
    H.place(p, ptrs, 1024)
    p.x_lo = 1 << 20
    H.each_null(lib, call, p, ptrs, b'null operand')
    p.x_lo = None
    assert call() == E_ARG and b'three products need x_lo' in err(lib)
    p.x_lo = 1 << 20
    for k in ('g', 'x', 'hw', 'out'):
        for q in ('g', 'x', 'hw', 'out'):
            setattr(p, f'{q}_plane_stride', 24)
        setattr(p, f'{k}_plane_stride', 23)
        assert call() == E_ARG and b'plane stride' in err(lib), k
    p.out_plane_stride = 24
    for k in ('g_hi', 'x_hi', 'hw_hi'):
        keep, p.out_hi = p.out_hi, getattr(p, k)
        assert call() == E_ARG and b'out must not be' in err(lib), k
        p.out_hi = keep
    H.each_misaligned(lib, call, p, ptrs + ('g_lo', 'x_lo', 'hw_lo', 'out_lo'), at=(1 << 21) + 8, message=b'16-byte aligned')
    # the two compiled pairs are (bf16, 3 products) and (fp16, 1 product): the others are refused by name
    p.products = 1
    assert call() == E_UNSUPPORTED and b'compiled for bf16 planes with three products' in err(lib)
    p.fmt, p.products = PF_F16, 3
    assert call() == E_UNSUPPORTED and b'compiled for bf16 planes with three products' in err(lib)


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
    assert lib.rsa_figsr_input(None, None) == E_ARG and b'null params' in err(lib)
    p = LF.FigsrInputParams()
    call = H.caller(lib.rsa_figsr_input, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.C, p.src_h, p.src_w, p.pad = 1, 3, 6, 7, 4
    H.each_bad(lib, call, p, (('batch', 0), ('C', 0), ('src_h', 0), ('src_w', 0), ('reserved0', 1)), E_ARG, b'geometry')
    p.C = 9
    assert call() == E_UNSUPPORTED and b'at most 8 channels' in err(lib)
    p.C = 3
    for h, w, pad in ((5, 6, 4), (6, 5, 4), (4, 8, 4), (8, 4, 4), (6, 6, -1)):  # 4 + size % 2 must stay below the size
        p.src_h, p.src_w, p.pad = h, w, pad
        assert call() == E_ARG and b'the reflection needs' in err(lib), (h, w, pad)
    p.src_h, p.src_w, p.pad, p.dtype = 6, 7, 4, L.U8
    assert call() == E_ARG and b'bad dtype' in err(lib)
    p.dtype, p.fmt = L.F32, 2
    assert call() == E_ARG and b'plane format' in err(lib)
    p.fmt = PF_BF16
    ptrs = ('x', 'shift', 'scale_norm', 'out_hi')
    for k in ptrs:
        setattr(p, k, 64)
    H.each_null(lib, call, p, ptrs, b'null operand')
    H.each_misaligned(lib, call, p, ('out_hi', 'out_lo'), at=72, message=b'16-byte aligned')
    p.out_plane_stride = 14 * 16 - 1  # 6 x 7 pads to 14 x 16
    assert call() == E_ARG and b'plane stride' in err(lib)


def test_output_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_figsr_output(None, None) == E_ARG and b'null params' in err(lib)
    p = LF.FigsrOutputParams()
    call = H.caller(lib.rsa_figsr_output, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.C, p.H, p.W, p.y0, p.x0, p.out_h, p.out_w = 1, 3, 28, 32, 8, 8, 12, 14
    H.each_bad(lib, call, p, (('batch', 0), ('C', 0), ('H', 0), ('W', 0), ('out_h', 0), ('out_w', 0), ('reserved0', 1)), E_ARG, b'geometry')
    H.each_bad(lib, call, p, (('y0', -1), ('x0', -1), ('y0', 17), ('x0', 19), ('out_h', 21), ('out_w', 25)), E_ARG, b'window leaves the map')
    p.dtype = L.U8
    assert call() == E_ARG and b'bad dtype' in err(lib)
    p.dtype = L.F16
    ptrs = ('y', 'shift', 'scale_norm', 'out')
    for k in ptrs:
        setattr(p, k, 64)
    H.each_null(lib, call, p, ptrs, b'null operand')


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
