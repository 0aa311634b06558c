"""include/resselt_amd_moesr.h against its ctypes mirror and signature row (resselt_amd/engine/lib_moesr.py): the same struct with the same
fields in the same order and type classes, the same prototype argument by argument, the symbol exported and typed by ``lib.load()``, and
the argument checks that need no GPU.  The comparisons are those tests/test_pack_and_capi.py and tests/test_capi_signatures.py make for
include/resselt_amd.h, which this header extends and whose tables it leaves alone."""

import ctypes
import os
import re

import pytest

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_moesr as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCT, ENTRY = 'rsa_moesr_stream_params', 'rsa_moesr_stream'


def _header():
    text = open(os.path.join(ROOT, 'include', 'resselt_amd_moesr.h')).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _header_structs():
    """{struct: [(field, 'int32_t' | 'int64_t' | 'float' | 'pointer')]} of every typedef struct in the header."""
    out = {}
    for name, body, closing in re.findall(r'typedef\s+struct\s+(rsa_\w+)\s*\{(.*?)\}\s*(\w+)\s*;', _header(), flags=re.S):
        assert closing == name
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            m = re.fullmatch(r'(?:const\s+)?(\w+)\b(.*)', decl, flags=re.S)
            assert m, f'{name}: cannot parse {decl!r}'
            for item in (i.strip() for i in m.group(2).split(',')):
                if '*' in item:
                    fields.append((item.replace('*', '').strip(), 'pointer'))
                else:
                    assert m.group(1) in ('int32_t', 'int64_t', 'float') and re.fullmatch(r'\w+', item), f'{name}: cannot parse {decl!r}'
                    fields.append((item, m.group(1)))
        out[name] = fields
    return out


def _header_prototypes():
    """{entry point: (return type, [(parameter, 'ptr' | the params struct a pointer points to | the scalar type)])}."""
    text = re.sub(r'typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;', '', _header(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r'(\w+)\s+(rsa_\w+)\s*\(([^)]*)\)\s*;', text):
        plist = []
        for p in params.split(','):
            m = re.fullmatch(r'(.*?)(\w+)', p.strip(), flags=re.S)
            words = [w for w in m.group(1).replace('*', ' * ').split() if w != 'const']
            plist.append((m.group(2), (words[0] if re.fullmatch(r'rsa_\w+_params', words[0]) else 'ptr') if '*' in words else words[0]))
        out[name] = (ret, plist)
    return out


def test_the_struct_matches_its_mirror():
    header = _header_structs()
    assert list(header) == [STRUCT]
    classes = {ctypes.c_int32: 'int32_t', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float', ctypes.c_void_p: 'pointer'}
    assert STRUCT in LM.MoesrStreamParams.__doc__
    assert [(k, classes[t]) for k, t in LM.MoesrStreamParams._fields_] == header[STRUCT]
    assert ctypes.sizeof(LM.MoesrStreamParams) == 8 * 4 + 7 * 8 + 2 * 4 + 4 * 8  # no padding: the C compiler lays it out the same way


def test_the_prototype_matches_its_row():
    header = _header_prototypes()
    assert list(header) == [ENTRY] == list(LM.SIGNATURES)
    restype, params = LM.SIGNATURES[ENTRY]
    assert restype is ctypes.c_int and header[ENTRY][0] == 'int'
    assert [(k, STRUCT if t is ctypes.POINTER(LM.MoesrStreamParams) else {ctypes.c_void_p: 'ptr'}[t]) for k, t in params] == header[ENTRY][1]


def test_the_main_tables_do_not_know_it_and_the_library_does():
    assert ENTRY not in L.SIGNATURES and ENTRY not in L.EXPORTS and L.EXTENSIONS[ENTRY] is LM.SIGNATURES[ENTRY]
    assert '#include "resselt_amd.h"' in open(os.path.join(ROOT, 'include', 'resselt_amd_moesr.h')).read()  # its conventions and enums
    lib = L.load()
    fn = getattr(lib, ENTRY)
    assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.POINTER(LM.MoesrStreamParams), ctypes.c_void_p]
    with pytest.raises(ValueError, match='entry points of include/resselt_amd.h'):
        L.extend({'rsa_layernorm': LM.SIGNATURES[ENTRY]})
    assert 'rsa_layernorm' not in L.EXTENSIONS


def test_argument_validation_without_gpu():
    lib = L.load()
    assert lib.rsa_moesr_stream(None, None) == -1 and b'null params' in lib.rsa_last_error_string()
    p = LM.MoesrStreamParams()
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'geometry' in lib.rsa_last_error_string()
    p.batch, p.H, p.W, p.C, p.mode, p.a_H, p.a_W = 1, 4, 4, 12, 0, 4, 4
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'multiple of 8' in lib.rsa_last_error_string()
    p.C, p.mode, p.a_H = 8, 1, 7
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'odd source size' in lib.rsa_last_error_string()
    p.mode, p.a_H = 0, 4
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -1 and b'null operand' in lib.rsa_last_error_string()
    p.a, p.gamma, p.s_in, p.s_out = 16, 16, 16, 24
    assert lib.rsa_moesr_stream(ctypes.byref(p), None) == -3  # misaligned pointer
