"""Every header under include/ against its ctypes description (``lib.HEADERS``: the rows table of each header; the mirrors are those of the
module that holds the table): the same prototypes argument by argument in the same order, the same structs field by field, no padding in
an extension's mirrors, the same constants, no name in two tables, and every row exported and typed by ``lib.load()``.  Everything but
the last reads the headers and the tables only: neither the library nor a GPU.  The parsers are in tests/capi_header.py."""

import copy
import ctypes
import re
import sys

import pytest

import capi_header as H
import resselt_amd  # noqa: F401  (registers every extension header)
from resselt_amd.engine import lib as L

MAIN = 'resselt_amd.h'
# prototypes / structs per header: a parser that quietly sees less fails here.  A new header adds its line.
COUNTS = {
    'resselt_amd.h': (106, 37),
    'resselt_amd_figsr.h': (4, 3),
    'resselt_amd_gaterv2.h': (2, 1),
    'resselt_amd_gaterv3.h': (6, 4),
    'resselt_amd_gfisr.h': (4, 2),
    'resselt_amd_gfisr1.h': (2, 2),
    'resselt_amd_lawfft.h': (6, 5),
    'resselt_amd_moesr.h': (1, 1),
    'resselt_amd_smosr.h': (3, 3),
}
# The headers whose comments name another family, because they build on its entry points (FIGSR and LAWFFT run rsa_gfisr_dft; GFISR v1
# joins the GFISR family and declares rsa_gfisr_ln_spectral; SMoSR's header points at MoESR's for its conventions).  No other header
# mentions a family that is not its own, in code or in comments.
CITES = {
    'resselt_amd_figsr.h': {'gfisr'},
    'resselt_amd_gfisr1.h': {'gfisr'},
    'resselt_amd_lawfft.h': {'figsr', 'gfisr'},
    'resselt_amd_smosr.h': {'moesr'},
}
FILES = H.header_files()
EXTENSION_FILES = [h for h in FILES if h != MAIN]


def _module(header):
    """The module that holds the rows table of ``header``, and with it the mirrors of the header's structs."""
    found = [m for m in list(sys.modules.values()) if getattr(m, 'SIGNATURES', None) is L.HEADERS[header]]
    assert len(found) == 1, (header, found)
    return found[0]


def _family(header):
    return header[len('resselt_amd_') : -len('.h')]


def test_registered_headers_are_the_files_in_include():
    assert not set(FILES) - set(L.HEADERS), f'no rows are registered for {sorted(set(FILES) - set(L.HEADERS))}'
    assert not set(L.HEADERS) - set(FILES), f'rows without a header in include/: {sorted(set(L.HEADERS) - set(FILES))}'
    assert set(FILES) == set(COUNTS) and len(FILES) == 9
    assert list(L.HEADERS)[0] == MAIN and L.HEADERS[MAIN] is L.SIGNATURES and L.EXPORTS == tuple(L.SIGNATURES)
    for header in EXTENSION_FILES:
        assert '#include "resselt_amd.h"' in H.text(header), header  # its conventions and enums
    totals = [sum(n) for n in zip(*COUNTS.values())]
    assert totals == [134, 58]


@pytest.mark.parametrize('header', FILES)
def test_prototypes_match_the_rows(header):
    protos = H.prototypes(header)
    assert len(protos) == COUNTS[header][0]
    assert set(protos) == H.declared(header) == set(L.HEADERS[header])  # the looser scan: no multi-line prototype was skipped
    assert ctypes.c_int is ctypes.c_int32  # status returns are declared `int`
    assert H.prototype_mismatches(header, L.HEADERS[header]) == []
    assert list(protos) == list(L.HEADERS[header])


@pytest.mark.parametrize('header', FILES)
def test_structs_match_the_mirrors(header):
    """The same structs, the same field names in the same order, the same type classes."""
    found, header_structs = H.mirrors(_module(header)), H.structs(header)
    assert len(header_structs) == COUNTS[header][1]
    assert H.struct_mismatches(header, found) == []
    if header == MAIN:
        assert 'rsa_conv_params' in found  # (engine/lib.py orders its mirrors in its own way)
    else:
        assert list(found) == list(header_structs)
        for name, mirror in found.items():  # no padding: the C compiler lays it out the same way
            assert ctypes.sizeof(mirror) == sum(ctypes.sizeof(t) for _, t in mirror._fields_), name


@pytest.mark.parametrize('header', EXTENSION_FILES)
def test_extension_names_stay_out_of_the_other_tables(header):
    rows = L.HEADERS[header]
    for name, row in rows.items():
        assert name not in L.SIGNATURES and name not in L.EXPORTS
        assert L.EXTENSIONS[name] is row and L.signature(name) is row
        assert [h for h, table in L.HEADERS.items() if name in table] == [header]
    names = set(H.prototypes(header)) | set(H.structs(header)) | set(H.defines(header))
    for other in FILES:
        if other != header:
            assert not names & (set(H.prototypes(other)) | set(H.structs(other)) | set(H.defines(other))), other
            assert (re.search(_family(header), H.text(other), flags=re.I) is not None) == (_family(header) in CITES.get(other, ())), other


def test_the_main_rows_stay_the_main_rows():
    assert L.signature('rsa_gated_dwconv') is L.SIGNATURES['rsa_gated_dwconv'] and 'rsa_gated_dwconv' not in L.EXTENSIONS
    gate = L.HEADERS['resselt_amd_gfisr.h']['rsa_gfisr_gate']
    assert gate[1][0][1] is L.SIGNATURES['rsa_gated_dwconv'][1][0][1]  # an extension may take a main-header descriptor: rsa_gated_dwconv_params, unchanged


@pytest.mark.parametrize('header', EXTENSION_FILES)
def test_constants_match(header):
    prefix = f'RSA_{_family(header).upper()}_'
    consts = H.defines(header)
    assert all(k.startswith(prefix) for k in consts), consts
    module = _module(header)
    assert consts == {k: getattr(module, k[len(prefix) :], None) for k in consts}


def test_the_constants_of_today():
    assert H.defines('resselt_amd_gaterv2.h') == {'RSA_GATERV2_TOKEN_CHUNK': 128}
    assert set(H.defines('resselt_amd_gaterv3.h')) == {'RSA_GATERV3_TILE_W', 'RSA_GATERV3_TILE_H', 'RSA_GATERV3_TOKEN_CHUNK'}
    assert H.defines(MAIN)['RSA_VERSION'] == 400 and H.defines(MAIN)['RSA_E_ALIGN'] == H.E_ALIGN  # a bare and a parenthesised value


@pytest.mark.parametrize('header', FILES)
def test_the_library_exports_and_types_every_row(header):
    assert H.declared(header), 'no prototypes parsed from the header'
    raw = ctypes.CDLL(L.lib_path())
    for name in H.declared(header):
        assert hasattr(raw, name), name
    lib = L.load()
    for name, (restype, params) in L.HEADERS[header].items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == [t for _, t in params], name
    assert lib.rsa_version() == 400


def test_the_comparison_rejects_a_dropped_argument_and_swapped_names():
    """One ``i32`` less in one row shifts every later argument; two names swapped in another reorder two equal-typed arguments; the same
    in a row of an extension header and in a mirror: none shows at import, all must show here, by name.  (On copies: the tables and the
    mirrors themselves are not touched.)"""
    table = copy.deepcopy(L.SIGNATURES)
    restype, params = table['rsa_rha_gate']
    i = [k for k, _ in params].index('i_planes')
    table['rsa_rha_gate'] = (restype, params[:i] + params[i + 1 :])
    restype, params = table['rsa_scale_add']
    names = [k for k, _ in params]
    a, b = names.index('res'), names.index('gamma')
    params[a], params[b] = params[b], params[a]
    bad = H.prototype_mismatches(MAIN, table)
    assert len(bad) == 2 and bad[0].startswith('rsa_rha_gate:') and bad[1].startswith('rsa_scale_add:')
    assert H.prototype_mismatches(MAIN, L.SIGNATURES) == []

    header = 'resselt_amd_gaterv3.h'
    table = dict(L.HEADERS[header])
    restype, params = table['rsa_gaterv3_attn_workspace_bytes']
    table['rsa_gaterv3_attn_workspace_bytes'] = (restype, [kt for kt in params if kt[0] != 'heads'])
    bad = H.prototype_mismatches(header, table)
    assert len(bad) == 1 and bad[0].startswith('rsa_gaterv3_attn_workspace_bytes:')
    moved = {k: L.HEADERS[header][k] for k in reversed(L.HEADERS[header])}  # every row right, the order wrong
    assert H.prototype_mismatches(header, moved) == [f'{header}: the table is not in the order of the header']

    found = H.mirrors(_module(header))
    real = found['rsa_gaterv3_shortcut_params']
    fields = list(real._fields_)
    a, b = [k for k, _ in fields].index('gamma'), [k for k, _ in fields].index('out')
    fields[a], fields[b] = fields[b], fields[a]
    swapped = type('Swapped', (ctypes.Structure,), {'__doc__': real.__doc__, '_fields_': fields})
    assert ctypes.sizeof(swapped) == ctypes.sizeof(real)  # nothing but the comparison can tell them apart
    bad = H.struct_mismatches(header, {**found, 'rsa_gaterv3_shortcut_params': swapped})
    assert len(bad) == 1 and bad[0].startswith('rsa_gaterv3_shortcut_params:')
    assert H.struct_mismatches(header, found) == []


@pytest.mark.parametrize('taken,owner', [('rsa_layernorm', 'resselt_amd.h'), ('rsa_smosr_pad', 'resselt_amd_smosr.h')])
def test_extend_refuses_a_name_another_header_holds(taken, owner):
    headers, extensions = dict(L.HEADERS), dict(L.EXTENSIONS)
    row = L.HEADERS['resselt_amd_moesr.h']['rsa_moesr_stream']
    with pytest.raises(ValueError, match=f'{taken}.* are entry points of include/{owner}'):
        L.extend({'rsa_new_entry': row, taken: row}, 'resselt_amd_new.h')
    assert L.HEADERS == headers and L.EXTENSIONS == extensions and list(L.HEADERS) == list(headers)
    assert 'rsa_new_entry' not in L.EXTENSIONS and taken not in L.HEADERS['resselt_amd_moesr.h']
