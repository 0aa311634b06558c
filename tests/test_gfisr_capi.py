"""The argument checks of ``rsa_gfisr_ln_spectral`` and ``rsa_plane_window`` (include/resselt_amd_gfisr1.h) that need no GPU: each returns
before any launch.  tests/test_capi_headers.py compares the header with its ctypes mirrors and rows (resselt_amd/engine/lib_gfisr1.py)."""

import capi_header as H
from capi_header import E_ALIGN, E_ARG, E_UNSUPPORTED, err
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gfisr1 as LG1


def test_ln_spectral_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_gfisr_ln_spectral(None, None) == E_ARG and b'null params' in err(lib)
    p = LG1.GfisrLnSpectralParams()
    call = H.caller(lib.rsa_gfisr_ln_spectral, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.H, p.W, p.C, p.eps = 1, 4, 4, 12, 1e-6
    H.each_bad(lib, call, p, (('reserved0', 1), ('batch', 0), ('batch', 65536), ('H', 0), ('W', 0), ('C', 0), ('eps', 0.0)), E_ARG, b'geometry')
    H.each_bad(lib, call, p, [('C', c) for c in (1, 3, 31, 33, 34, 64)], E_UNSUPPORTED, b'even and in 2..32')
    ptrs = ('x', 'ln_w', 'ln_b', 'fpe_w', 'fpe_b', 'fdc_w', 'fdc_b', 'out')
    H.place(p, ptrs, 64)
    H.each_null(lib, call, p, ptrs, b'null pointer')
    H.each_misaligned(lib, call, p, ptrs, by=8)
    p.out = p.x
    assert call() == E_ARG and b'must not overlap' in err(lib)


def test_plane_window_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_plane_window(None, None) == E_ARG and b'null params' in err(lib)
    p = LG1.PlaneWindowParams()
    call = H.caller(lib.rsa_plane_window, p)
    assert call() == E_ARG and b'geometry' in err(lib)
    p.batch, p.planes, p.H, p.W, p.out_H, p.out_W, p.top, p.left = 1, 2, 5, 4, 10, 8, 2, 2
    H.each_bad(lib, call, p, [(key, 0) for key in ('batch', 'planes', 'H', 'W', 'out_H', 'out_W')], E_ARG, b'geometry')
    assert call() == E_ARG and b'null pointer' in err(lib)
    p.in_hi, p.out_hi = 64, 128
    p.in_lo = 256
    assert call() == E_ARG and b'go together' in err(lib)
    p.in_lo, p.out_lo = None, 256
    assert call() == E_ARG and b'go together' in err(lib)
    p.in_lo = 512
    H.each_misaligned(lib, call, p, ('in_hi', 'in_lo', 'out_hi', 'out_lo'), by=4)
    p.in_plane_stride, p.out_plane_stride = 19, 80
    assert call() == E_ARG and b'plane stride' in err(lib)
    p.in_plane_stride, p.out_plane_stride = 20, 79
    assert call() == E_ARG and b'plane stride' in err(lib)
    p.out_plane_stride = 400
    # torch's rule: a pad must stay below the side -- an index may reflect once, never twice
    H.each_bad(lib, call, p, (('top', 5), ('left', 4), ('out_H', 2 + 2 * 4 + 2), ('out_W', 2 + 2 * 3 + 2), ('top', -6), ('H', 2)), E_ARG, b'second reflection')
