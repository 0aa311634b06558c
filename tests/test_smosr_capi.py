"""include/resselt_amd_smosr.h against its ctypes mirrors and signature rows (resselt_amd/engine/lib_smosr.py): the same structs with the
same fields in the same order and type classes, the same prototypes argument by argument, the symbols exported and typed by
``lib.load()``, and the argument checks that need no GPU.  The comparisons are those of tests/test_moesr_capi.py (whose parsers these
are), which tests/test_pack_and_capi.py and tests/test_capi_signatures.py make for include/resselt_amd.h."""

import ctypes
import os

import pytest

import test_moesr_capi as M
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_smosr as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'resselt_amd_smosr.h')
MIRRORS = {'rsa_smosr_gate_params': LS.SmosrGateParams, 'rsa_smosr_pad_params': LS.SmosrPadParams, 'rsa_smosr_pa_params': LS.SmosrPaParams}
ENTRIES = {'rsa_smosr_gate': 'rsa_smosr_gate_params', 'rsa_smosr_pad': 'rsa_smosr_pad_params', 'rsa_smosr_pa': 'rsa_smosr_pa_params'}
SIZES = {'rsa_smosr_gate_params': 6 * 4 + 4 * 8 + 4 * 8, 'rsa_smosr_pad_params': 8 * 4 + 8 + 4 * 8, 'rsa_smosr_pa_params': 8 * 4 + 2 * 8 + 8 * 8}


@pytest.fixture(autouse=True)
def _this_header(monkeypatch):
    """test_moesr_capi's parsers read ``_header()``: point it at this family's header."""
    import re

    text = open(HEADER).read()
    monkeypatch.setattr(M, '_header', lambda: re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))


def test_the_structs_match_their_mirrors():
    header = M._header_structs()
    assert list(header) == list(MIRRORS)
    classes = {ctypes.c_int32: 'int32_t', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float', ctypes.c_void_p: 'pointer'}
    for name, mirror in MIRRORS.items():
        assert name in mirror.__doc__
        assert [(k, classes[t]) for k, t in mirror._fields_] == header[name], name
        assert ctypes.sizeof(mirror) == SIZES[name], name  # no padding: the C compiler lays it out the same way


def test_the_prototypes_match_their_rows():
    header = M._header_prototypes()
    assert list(header) == list(ENTRIES) == list(LS.SIGNATURES)
    for entry, struct in ENTRIES.items():
        restype, params = LS.SIGNATURES[entry]
        assert restype is ctypes.c_int and header[entry][0] == 'int'
        assert [(k, struct if t is ctypes.POINTER(MIRRORS[struct]) else {ctypes.c_void_p: 'ptr'}[t]) for k, t in params] == header[entry][1]


def test_the_main_tables_do_not_know_them_and_the_library_does():
    assert '#include "resselt_amd.h"' in open(HEADER).read()  # its conventions and enums
    lib = L.load()
    for entry, struct in ENTRIES.items():
        assert entry not in L.SIGNATURES and entry not in L.EXPORTS and L.EXTENSIONS[entry] is LS.SIGNATURES[entry]
        fn = getattr(lib, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.POINTER(MIRRORS[struct]), ctypes.c_void_p]
    main = open(os.path.join(ROOT, 'include', 'resselt_amd.h')).read()
    assert 'smosr' not in main


def _rc(fn, p, code, text):
    lib = L.load()
    rc = fn(ctypes.byref(p), None)
    msg = lib.rsa_last_error_string()
    assert rc == code and text in msg, (rc, msg)


def test_gate_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_smosr_gate(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LS.SmosrGateParams()
    _rc(lib.rsa_smosr_gate, p, -1, b'geometry')
    p.batch, p.H, p.W, p.C = 1, 4, 4, 12
    _rc(lib.rsa_smosr_gate, p, -1, b'multiple of 8')
    p.C = 136
    _rc(lib.rsa_smosr_gate, p, -1, b'multiple of 8')
    p.C, p.fmt = 8, 2
    _rc(lib.rsa_smosr_gate, p, -1, b'plane format')
    p.fmt = 0
    _rc(lib.rsa_smosr_gate, p, -1, b'null operand')
    p.a, p.s_in = 64, 128
    _rc(lib.rsa_smosr_gate, p, -1, b'no output')
    p.out_lo = 256
    _rc(lib.rsa_smosr_gate, p, -1, b'no output')
    p.s_out = 64
    _rc(lib.rsa_smosr_gate, p, -1, b'out_lo without out_hi')
    p.out_lo = None
    _rc(lib.rsa_smosr_gate, p, -1, b's_out must not be a')
    p.s_out = 128  # in place on s_in: legal; the next refusal is the alignment
    p.s2_in = 24
    _rc(lib.rsa_smosr_gate, p, -3, b'16-byte aligned')
    p.s2_in, p.out_hi, p.out_plane_stride = None, 512, 15
    _rc(lib.rsa_smosr_gate, p, -1, b'plane stride')
    p.reserved0, p.out_plane_stride = 1, 16
    _rc(lib.rsa_smosr_gate, p, -1, b'reserved0')


def test_pad_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_smosr_pad(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LS.SmosrPadParams()
    _rc(lib.rsa_smosr_pad, p, -1, b'geometry')
    p.batch, p.C, p.src_h, p.src_w, p.pad = 1, 3, 2, 9, 2
    _rc(lib.rsa_smosr_pad, p, -1, b'reflection needs')
    p.src_h, p.dtype = 3, L.U8  # 8-bit images are not a source of this entry point
    _rc(lib.rsa_smosr_pad, p, -1, b'bad dtype')
    p.dtype = 0
    _rc(lib.rsa_smosr_pad, p, -1, b'null operand')
    p.x, p.out_hi = 4, 24
    _rc(lib.rsa_smosr_pad, p, -3, b'16-byte aligned')
    p.out_hi, p.out_plane_stride = 32, 7 * 13 - 1
    _rc(lib.rsa_smosr_pad, p, -1, b'plane stride')


def test_pa_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_smosr_pa(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LS.SmosrPaParams()
    _rc(lib.rsa_smosr_pa, p, -1, b'geometry')
    p.batch, p.H, p.W, p.C = 1, 3, 5, 20
    _rc(lib.rsa_smosr_pa, p, -1, b'multiple of 8')
    p.C, p.products = 24, 2
    _rc(lib.rsa_smosr_pa, p, -1, b'products must be 1 or 3')
    p.products = 3
    _rc(lib.rsa_smosr_pa, p, -1, b'null operand')
    p.w_frag, p.bias, p.in_hi, p.out_hi = 16, 32, 64, 1024
    _rc(lib.rsa_smosr_pa, p, -1, b'need in_lo')
    p.in_lo = 2048 + 8
    _rc(lib.rsa_smosr_pa, p, -3, b'16-byte aligned')
    p.in_lo, p.in_plane_stride, p.out_plane_stride = 2048, 15, 14
    _rc(lib.rsa_smosr_pa, p, -1, b'plane stride')
    p.out_plane_stride, p.out_hi = 16, 64  # in place with another stride
    _rc(lib.rsa_smosr_pa, p, -1, b'in place needs equal strides')
    p.out_plane_stride, p.out_lo = 15, 4096  # ... or with another lo buffer
    _rc(lib.rsa_smosr_pa, p, -1, b'in place needs equal strides')
