"""The argument checks of ``rsa_smosr_gate``, ``rsa_smosr_pad`` and ``rsa_smosr_pa`` (include/resselt_amd_smosr.h) that need no GPU: each
returns before any launch.  tests/test_capi_headers.py compares the header with its ctypes mirrors and rows
(resselt_amd/engine/lib_smosr.py)."""

import capi_header as H
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_smosr as LS


def test_gate_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_smosr_gate(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LS.SmosrGateParams()
    call = H.caller(lib.rsa_smosr_gate, p)
    H.refuses(lib, call, -1, b'geometry')
    p.batch, p.H, p.W, p.C = 1, 4, 4, 12
    H.refuses(lib, call, -1, b'multiple of 8')
    p.C = 136
    H.refuses(lib, call, -1, b'multiple of 8')
    p.C, p.fmt = 8, 2
    H.refuses(lib, call, -1, b'plane format')
    p.fmt = 0
    H.refuses(lib, call, -1, b'null operand')
    p.a, p.s_in = 64, 128
    H.refuses(lib, call, -1, b'no output')
    p.out_lo = 256
    H.refuses(lib, call, -1, b'no output')
    p.s_out = 64
    H.refuses(lib, call, -1, b'out_lo without out_hi')
    p.out_lo = None
    H.refuses(lib, call, -1, b's_out must not be a')
    p.s_out = 128  # in place on s_in: legal; the next refusal is the alignment
    p.s2_in = 24
    H.refuses(lib, call, -3, b'16-byte aligned')
    p.s2_in, p.out_hi, p.out_plane_stride = None, 512, 15
    H.refuses(lib, call, -1, b'plane stride')
    p.reserved0, p.out_plane_stride = 1, 16
    H.refuses(lib, call, -1, b'reserved0')


def test_pad_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_smosr_pad(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LS.SmosrPadParams()
    call = H.caller(lib.rsa_smosr_pad, p)
    H.refuses(lib, call, -1, b'geometry')
    p.batch, p.C, p.src_h, p.src_w, p.pad = 1, 3, 2, 9, 2
    H.refuses(lib, call, -1, b'reflection needs')
    p.src_h, p.dtype = 3, L.U8  # 8-bit images are not a source of this entry point
    H.refuses(lib, call, -1, b'bad dtype')
    p.dtype = 0
    H.refuses(lib, call, -1, b'null operand')
    p.x, p.out_hi = 4, 24
    H.refuses(lib, call, -3, b'16-byte aligned')
    p.out_hi, p.out_plane_stride = 32, 7 * 13 - 1
    H.refuses(lib, call, -1, b'plane stride')


def test_pa_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_smosr_pa(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LS.SmosrPaParams()
    call = H.caller(lib.rsa_smosr_pa, p)
    H.refuses(lib, call, -1, b'geometry')
    p.batch, p.H, p.W, p.C = 1, 3, 5, 20
    H.refuses(lib, call, -1, b'multiple of 8')
    p.C, p.products = 24, 2
    H.refuses(lib, call, -1, b'products must be 1 or 3')
    p.products = 3
    H.refuses(lib, call, -1, b'null operand')
    p.w_frag, p.bias, p.in_hi, p.out_hi = 16, 32, 64, 1024
    H.refuses(lib, call, -1, b'need in_lo')
    p.in_lo = 2048 + 8
    H.refuses(lib, call, -3, b'16-byte aligned')
    p.in_lo, p.in_plane_stride, p.out_plane_stride = 2048, 15, 14
    H.refuses(lib, call, -1, b'plane stride')
    p.out_plane_stride, p.out_hi = 16, 64  # in place with another stride
    H.refuses(lib, call, -1, b'in place needs equal strides')
    p.out_plane_stride, p.out_lo = 15, 4096  # ... or with another lo buffer
    H.refuses(lib, call, -1, b'in place needs equal strides')
