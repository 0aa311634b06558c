"""The C-ABI headers under include/ and their ctypes descriptions, both read into the same plain shapes so that a test can compare them
(tests/test_capi_headers.py), and the walks the argument-validation tests of every family share.  A helper module like tests/helpers.py:
it reads header text, ctypes classes and rows tables, and calls an entry point only where a test hands it one.  A header this cannot
parse is an assertion failure, never a skip."""

import ctypes
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3  # RSA_E_ARG, RSA_E_UNSUPPORTED, RSA_E_ALIGN

_STRUCT = r'typedef\s+struct\s+(rsa_\w+)\s*\{(.*?)\}\s*(\w+)\s*;'
_FIELD_CLASSES = {ctypes.c_int32: 'int32_t', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float', ctypes.c_void_p: 'pointer'}
_ARG_CLASSES = {ctypes.c_int32: 'i32', ctypes.c_int64: 'i64', ctypes.c_float: 'f32', ctypes.c_void_p: 'ptr', ctypes.c_char_p: 'cstr'}


def header_files() -> list:
    return sorted(f for f in os.listdir(INCLUDE) if f.endswith('.h'))


def text(header_file: str) -> str:
    with open(os.path.join(INCLUDE, header_file)) as fh:
        return fh.read()


def code(header_file: str) -> str:
    """The header without its comments."""
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text(header_file), flags=re.S))


def structs(header_file: str) -> dict:
    """{struct: [(field, type class)]} of every ``typedef struct rsa_* { ... } rsa_*;`` in the header, in the header's order.  Type classes:
    'int32_t', 'int64_t', 'float', 'pointer', or ('array', element struct, length)."""
    out = {}
    for name, body, closing in re.findall(_STRUCT, code(header_file), flags=re.S):
        assert closing == name and name not in out, f'{header_file}: {name} / {closing}'
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            m = re.fullmatch(r'(?:const\s+)?(\w+)\b(.*)', decl, flags=re.S)
            assert m, f'{name}: cannot parse {decl!r}'
            ctype, rest = m.group(1), m.group(2)
            for item in (i.strip() for i in rest.split(',')):
                arr = re.fullmatch(r'(\w+)\s*\[\s*(\d+)\s*\]', item)
                if arr:
                    fields.append((arr.group(1), ('array', ctype, int(arr.group(2)))))
                elif '*' in item:
                    fields.append((item.replace('*', '').strip(), 'pointer'))
                else:
                    assert ctype in ('int32_t', 'int64_t', 'float') and re.fullmatch(r'\w+', item), f'{name}: cannot parse {decl!r}'
                    fields.append((item, ctype))
        out[name] = fields
    return out


def prototypes(header_file: str) -> dict:
    """{entry point: (return class, [(parameter, type class)])} of every prototype in the header, in the header's order.  Type classes:
    'i32' (int32_t, int, an enum), 'i64', 'f32', 'cstr' (char*), 'ptr' (any other pointer), or the name of the ``rsa_*_params`` struct a
    pointer points to."""
    body = re.sub(_STRUCT, '', code(header_file), flags=re.S)

    def type_class(decl: str) -> str:
        words = decl.replace('*', ' * ').split()
        base = [w for w in words if w not in ('const', '*', 'struct', 'enum')]
        assert len(base) == 1, decl
        if '*' in words:
            return 'cstr' if base[0] == 'char' else base[0] if re.fullmatch(r'rsa_\w+_params', base[0]) else 'ptr'
        return 'i32' if 'enum' in words else {'int': 'i32', 'int32_t': 'i32', 'int64_t': 'i64', 'float': 'f32'}[base[0]]

    out = {}
    for ret, name, params in re.findall(r'((?:const\s+)?\w+\s*\*?)\s*(rsa_\w+)\s*\(([^)]*)\)\s*;', body):
        assert name not in out, f'{name} is declared twice'
        plist = []
        if params.strip() not in ('', 'void'):
            for p in params.split(','):
                m = re.fullmatch(r'(.*?)(\w+)', p.strip(), flags=re.S)
                assert m, f'{name}: cannot parse {p!r}'
                plist.append((m.group(2), type_class(m.group(1))))
        out[name] = (type_class(ret), plist)
    return out


def declared(header_file: str) -> set:
    """The entry points a looser, line-by-line scan of the raw header sees: ``prototypes`` must not have skipped a multi-line one."""
    return set(re.findall(r'^\s*(?:const\s+)?(?:int|int64_t|char\s*\*|void)\s*\*?\s*(rsa_\w+)\s*\(', text(header_file), flags=re.M))


def defines(header_file: str) -> dict:
    """{name: value} of every ``#define RSA_<NAME> <integer>`` in the header (the value may stand in parentheses)."""
    return {k: int(v) for k, v in re.findall(r'^\s*#\s*define\s+(RSA_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$', code(header_file), flags=re.M)}


def _cited(mirror) -> str:
    """The ``struct rsa_*`` the docstring of a ctypes mirror cites."""
    m = re.search(r'struct (rsa_\w+)', mirror.__doc__ or '')
    assert m, f'{mirror.__name__} cites no struct'
    return m.group(1)


def mirrors(module) -> dict:
    """{struct: ctypes mirror} of every ``Structure`` that ``module`` defines, in the module's order."""
    out = {}
    for v in vars(module).values():
        if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == module.__name__:
            assert _cited(v) not in out, f'two mirrors of {_cited(v)}'
            out[_cited(v)] = v
    return out


def mirror_fields(mirror) -> list:
    """The fields of a ctypes mirror in the shape of ``structs``."""
    fields = []
    for name, ftype in mirror._fields_:
        if issubclass(ftype, ctypes.Array):
            fields.append((name, ('array', _cited(ftype._type_), ftype._length_)))
        else:
            fields.append(('in' if name == 'in_' else name, _FIELD_CLASSES[ftype]))  # `in` is a Python keyword
    return fields


def table_prototypes(rows: dict) -> dict:
    """A rows table (``lib.SIGNATURES``, or those of an extension) in the shape of ``prototypes``."""

    def type_class(t):
        return _ARG_CLASSES[t] if t in _ARG_CLASSES else _cited(t._type_)

    return {name: (type_class(restype), [(k, type_class(t)) for k, t in params]) for name, (restype, params) in rows.items()}


def prototype_mismatches(header_file: str, rows: dict) -> list:
    """One line per entry point on which the header and the rows table disagree, each starting with the entry point's name."""
    header, table = prototypes(header_file), table_prototypes(rows)
    bad = [f'{name}: only in the {"header" if name in header else "table"}' for name in sorted(set(header) ^ set(table))]
    bad += [f'{name}: header {header[name]} != table {table[name]}' for name in sorted(set(header) & set(table)) if header[name] != table[name]]
    if not bad and list(header) != list(table):
        bad.append(f'{header_file}: the table is not in the order of the header')
    return bad


def struct_mismatches(header_file: str, found: dict) -> list:
    """The same for the structs of the header and the ``mirrors`` of its module, each line starting with the struct's name."""
    header, mirror = structs(header_file), {name: mirror_fields(m) for name, m in found.items()}
    bad = [f'{name}: only in the {"header" if name in header else "module"}' for name in sorted(set(header) ^ set(mirror))]
    return bad + [f'{name}: header {header[name]} != mirror {mirror[name]}' for name in sorted(set(header) & set(mirror)) if header[name] != mirror[name]]


# ---- argument validation: the library refuses before any launch, so none of this needs a GPU ----
def err(lib) -> bytes:
    return lib.rsa_last_error_string()


def caller(fn, p):
    """``fn(&p, stream = NULL)`` as a call without arguments, for the walks below."""
    return lambda: fn(ctypes.byref(p), None)


def refuses(lib, call, status: int, message: bytes = b'', what=None) -> None:
    rc = call()
    assert rc == status and message in err(lib), (what, rc, err(lib))


def place(p, names, step: int) -> None:
    """Distinct addresses for the pointer fields ``names``: step, 2 step, ..."""
    for i, k in enumerate(names):
        setattr(p, k, step * (i + 1))


def each_null(lib, call, p, names, message: bytes) -> None:
    """Every required pointer NULL in turn: RSA_E_ARG and ``message``."""
    for k in names:
        keep = getattr(p, k)
        setattr(p, k, None)
        refuses(lib, call, E_ARG, message, k)
        setattr(p, k, keep)


def each_misaligned(lib, call, p, names, at=None, by: int = 8, message: bytes = b'') -> None:
    """Every listed pointer off a 16-byte boundary in turn (moved ``by`` bytes, or set to address ``at``): RSA_E_ALIGN."""
    for k in names:
        keep = getattr(p, k)
        setattr(p, k, keep + by if at is None else at)
        refuses(lib, call, E_ALIGN, message, k)
        setattr(p, k, keep)


def each_bad(lib, call, p, pairs, status: int, message: bytes) -> None:
    """Every ``(field, bad value)`` in turn: ``status`` and ``message``; the field has its value back afterwards."""
    for key, bad in pairs:
        keep = getattr(p, key)
        setattr(p, key, bad)
        refuses(lib, call, status, message, (key, bad))
        setattr(p, key, keep)
