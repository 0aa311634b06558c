"""The keyword binder built on ``lib.SIGNATURES`` (reads the table only: neither the library nor a GPU).  tests/test_capi_headers.py compares
the table with the prototypes of include/resselt_amd.h."""

import ctypes

import pytest

from resselt_amd.engine import lib as L


class _FakePlanes:
    """What ``bind`` reads of a ``Planes`` buffer: 100 bytes per plane, lo halves 5000 bytes behind the hi halves (or none)."""

    plane_stride, batch_stride = 7, 21

    def __init__(self, base, with_lo=True):
        self.base, self.with_lo = base, with_lo

    def hi_ptr(self, plane=0):
        return self.base + 100 * plane

    def lo_ptr(self, plane=0):
        return self.base + 5000 + 100 * plane if self.with_lo else None


class _FakeTensor:
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


@pytest.fixture
def fake_entry(monkeypatch):
    sig = (ctypes.c_int, L._ptr('x') + L._plane_fields('in') + L._i32('batch', 'n') + L._f32('eps') + L._plane_fields('out') + L._ptr('aux', 'stream'))
    monkeypatch.setitem(L.SIGNATURES, 'rsa_fake', sig)
    return 'rsa_fake'


def test_bind_expands_planes_tensors_and_none(fake_entry):
    src, dst = _FakePlanes(10000), _FakePlanes(20000, with_lo=False)
    args = L.bind(fake_entry, x=_FakeTensor(77), in_=src, batch=2, n=5, eps=0.5, out=(dst, 3), aux=None)
    assert args == [77, 10000, 15000, 7, 21, 2, 5, 0.5, 20300, None, 7, 21, None]  # the header's order, the stream left to the caller
    # a plane offset moves both halves; keyword order does not matter
    args = L.bind(fake_entry, aux=_FakeTensor(9), out=dst, eps=1.0, n=1, batch=1, **{'in': (src, 2)}, x=None)
    assert args == [None, 10200, 15200, 7, 21, 1, 1, 1.0, 20000, None, 7, 21, 9]


def test_bind_lo_override_and_header_named_scalars(fake_entry):
    src, dst = _FakePlanes(10000), _FakePlanes(20000)
    common = dict(x=None, batch=1, n=1, eps=0.0, aux=None)
    assert L.bind(fake_entry, in_=src, in_lo=None, out=dst, **common)[1:5] == [10000, None, 7, 21]  # a reader that must not see lo halves
    assert L.bind(fake_entry, in_=src, out=dst, out_lo=12345, **common)[8:10] == [20000, 12345]
    # an operand given by its four header names instead of a buffer
    args = L.bind(fake_entry, in_=src, out_hi=1, out_lo=2, out_plane_stride=3, out_batch_stride=4, **common)
    assert args[8:12] == [1, 2, 3, 4]


def test_bind_raises_before_anything_is_launched(fake_entry):
    src, dst = _FakePlanes(10000), _FakePlanes(20000)
    good = dict(x=None, in_=src, batch=1, n=1, eps=0.0, out=dst, aux=None)
    assert len(L.bind(fake_entry, **good)) == 13
    with pytest.raises(TypeError, match=r"rsa_fake: missing parameter 'eps'"):
        L.bind(fake_entry, **{k: v for k, v in good.items() if k != 'eps'})
    with pytest.raises(TypeError, match=r"rsa_fake: missing parameter 'out_hi', 'out_lo', 'out_plane_stride', 'out_batch_stride'"):
        L.bind(fake_entry, **{k: v for k, v in good.items() if k != 'out'})
    with pytest.raises(TypeError, match=r"rsa_fake: no parameter 'epsilon'"):
        L.bind(fake_entry, **good, epsilon=1.0)
    with pytest.raises(TypeError, match=r"rsa_fake: no parameter 'y_hi'"):
        L.bind(fake_entry, **good, y=src)  # a buffer under a name that is no plane operand
    with pytest.raises(TypeError, match=r"rsa_fake: parameter 'in_hi' given twice"):
        L.bind(fake_entry, **good, in_hi=5)
    with pytest.raises(TypeError, match=r"rsa_fake: parameter 'stream' given twice"):
        L.bind(fake_entry, **good, stream=0)  # the caller of the entry point supplies it
    with pytest.raises(TypeError, match=r"rsa_fake: 'n' has a plane offset but is no plane buffer"):
        L.bind(fake_entry, **{**good, 'n': (4, 1)})


def test_bind_real_entry_points():
    f, kv, cat = _FakePlanes(10000), _FakePlanes(20000), _FakePlanes(30000)
    geo = dict(batch=2, H=8, W=16, fmt=L.PF_F16)
    # rsa_flex_gate_add, the last block of a group: the planes from plane 4 on, no f32 output
    args = L.bind('rsa_flex_gate_add', r=(f, 12), kv=kv, base_f32=_FakeTensor(1), out_f32=None, out=(cat, 4), C=32, **geo)
    assert args == [11200, 16200, 7, 21, 20000, 25000, 7, 21, 1, None, 30400, 35400, 7, 21, 2, 8, 16, 32, L.PF_F16]
    assert len(args) + 1 == len(L.SIGNATURES['rsa_flex_gate_add'][1])
    # rsa_gated_add names its plane operand x_hi / x_lo / plane_stride / batch_stride: given by those names
    args = L.bind('rsa_gated_add', x_hi=f.hi_ptr(), x_lo=f.lo_ptr(), plane_stride=f.plane_stride, batch_stride=f.batch_stride, batch=1, H=8, W=16, C=60,
                  gate=_FakeTensor(3), scale=0.01, base_f32=_FakeTensor(4), out_f32=_FakeTensor(5))  # fmt: skip
    assert args == [10000, 15000, 7, 21, 1, 8, 16, 60, 3, 0.01, 4, 5]
    with pytest.raises(TypeError, match=r"rsa_gated_add: no parameter 'x_plane_stride'"):
        L.bind('rsa_gated_add', x=f, batch=1, H=8, W=16, C=60, gate=None, scale=0.01, base_f32=None, out_f32=None)
    # a descriptor passes through to its pointer parameter
    p = L.DySampleParams()
    assert L.bind('rsa_dysample', p=p) == [p]
    assert L.bind('rsa_check_status') == [] and L.bind('rsa_conv_cout_tiles', cout=48) == [48]
