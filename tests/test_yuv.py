"""The video pixel formats of ``upscale_yuv`` on CPU tensors: the f32 torch path of ``ops.yuv420_to_nchw`` /
``ops.nchw_to_yuv420`` against the f64 definition (tests/yuv_reference.py), hand-checkable pins, ``upscale_yuv`` with fake models, the
refusals, and the argument checks of the two entry points (host only: nothing is launched).

Bounds (yuv_reference.py derives them): a value read is within ``B = 32 * 2^-24`` (plus one rounding of an f16 / bf16 destination) of the
f64 value, a written code within ``0.5 + 2^bits * B`` of the unrounded f64 target.  Where the frame that is written comes out of an f32 blend
sum or an f32 resampling, that step's own bound (tests/test_resample.py) is added, times 2^bits."""

import ctypes as C

import pytest
import torch

import resample_reference as R
import resselt_amd
import tile_blend_reference as TB
import yuv_reference as Y
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.tiling import plan_tiles, resample_table

COMBOS = [(f, m, r, c) for f in Y.FORMATS for m in Y.MATRICES for r in Y.RANGES for c in Y.CHROMA_LOCS]


def _kw(fmt, matrix, range, chroma_loc):
    return dict(fmt=fmt, matrix=matrix, range=range, chroma_loc=chroma_loc)


@pytest.mark.parametrize('fmt,matrix,range,chroma_loc', COMBOS)
def test_torch_path_reads_as_the_definition(fmt, matrix, range, chroma_loc):
    kw = _kw(fmt, matrix, range, chroma_loc)
    for n, h, w in ((2, 10, 14), (1, 2, 2)):
        y, uv = Y.random_planes(n, h, w, fmt, seed=h * w)
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            got = ops.yuv420_to_nchw(y, uv, dtype=dtype, **kw)
            assert got.dtype == dtype
            Y.assert_read(got, y, uv, f'torch read {kw} {n}x{h}x{w}', **kw)
    one = ops.yuv420_to_nchw(y[0], uv[0], dtype=torch.float32, **kw)  # [H, W] planes: a batch of one
    assert torch.equal(one, ops.yuv420_to_nchw(y[:1], uv[:1], dtype=torch.float32, **kw))


@pytest.mark.parametrize('fmt,matrix,range,chroma_loc', COMBOS)
def test_torch_path_writes_as_the_definition(fmt, matrix, range, chroma_loc):
    kw = _kw(fmt, matrix, range, chroma_loc)
    for n, h, w in ((2, 10, 14), (1, 2, 2)):
        x = Y.random_rgb(n, h, w, seed=h + w)
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            xs = x.to(dtype)
            assert torch.equal(xs.double().nan_to_num(7), x.double().nan_to_num(7))  # the values are exact in every format
            y, uv = ops.nchw_to_yuv420(xs, **kw)
            assert tuple(y.shape) == (n, h, w) and tuple(uv.shape) == (n, h // 2, w // 2, 2)
            Y.assert_written(y, uv, x, f'torch write {kw} {dtype} {n}x{h}x{w}', **kw)


@pytest.mark.parametrize('matrix', list(Y.MATRICES))
def test_limited_range_black_and_white(matrix):
    for fmt, m in (('nv12', 1), ('p010', 4)):
        dt = Y.FORMATS[fmt][1]
        for code, value in ((16, 0.0), (235, 1.0)):
            y = torch.full((1, 4, 6), code * m * (64 if m == 4 else 1), dtype=torch.int32).to(dt)
            uv = torch.full((1, 2, 3, 2), 128 * m * (64 if m == 4 else 1), dtype=torch.int32).to(dt)
            for ref in (ops.yuv420_to_nchw(y, uv, fmt, matrix, dtype=torch.float32).double(), Y.to_rgb64(y, uv, fmt, matrix)):
                assert (ref - value).abs().max().item() <= 2.0**-22
            rgb = torch.full((1, 3, 4, 6), value)
            gy, guv = ops.nchw_to_yuv420(rgb, fmt, matrix)
            assert torch.equal(gy, y) and torch.equal(guv, uv)


def test_bt709_limited_red():
    rgb = torch.zeros(1, 3, 4, 4)
    rgb[:, 0] = 1.0
    ty, tuv = Y.to_yuv64(rgb)
    assert torch.equal(ty.round(), torch.full_like(ty, 63)) and torch.equal(tuv.round()[..., 0], torch.full((1, 2, 2), 102.0, dtype=torch.float64))
    assert torch.equal(tuv.round()[..., 1], torch.full((1, 2, 2), 240.0, dtype=torch.float64))
    y, uv = ops.nchw_to_yuv420(rgb)
    assert y.dtype == torch.uint8 and set(y.flatten().tolist()) == {63} and set(uv[..., 0].flatten().tolist()) == {102} and set(uv[..., 1].flatten().tolist()) == {240}


@pytest.mark.parametrize('fmt,matrix,range,chroma_loc', COMBOS)
def test_a_constant_frame_survives_a_round_trip(fmt, matrix, range, chroma_loc):
    kw = _kw(fmt, matrix, range, chroma_loc)
    bits, dt = Y.FORMATS[fmt]
    m = 2 ** (bits - 8)
    shift = 6 if bits == 10 else 0
    for cy, cb, cr in ((100, 120, 140), (180, 128, 128), (60, 110, 135)):  # in gamut for every matrix: nothing is clamped
        y = torch.full((1, 6, 8), (cy * m) << shift, dtype=torch.int32).to(dt)
        uv = torch.tensor([(cb * m) << shift, (cr * m) << shift], dtype=torch.int32).to(dt).expand(1, 3, 4, 2).contiguous()
        rgb = ops.yuv420_to_nchw(y, uv, dtype=torch.float32, **kw)
        assert 0 < rgb.min().item() and rgb.max().item() < 1
        gy, guv = ops.nchw_to_yuv420(rgb, **kw)
        assert torch.equal(gy, y) and torch.equal(guv, uv), (kw, cy, cb, cr)


def test_p010_low_bits_are_ignored_on_read_and_zero_on_write():
    y, uv = Y.random_planes(1, 6, 8, 'p010', seed=5)
    assert int(Y.low_bits(y).max()) > 0
    clean = lambda t: ((t.to(torch.int32) >> 6) << 6).to(torch.uint16)  # noqa: E731
    a = ops.yuv420_to_nchw(y, uv, 'p010', dtype=torch.float32)
    assert torch.equal(a, ops.yuv420_to_nchw(clean(y), clean(uv), 'p010', dtype=torch.float32))
    gy, guv = ops.nchw_to_yuv420(a, 'p010')
    assert gy.dtype == torch.uint16 and int(Y.low_bits(gy).max()) == 0 and int(Y.low_bits(guv).max()) == 0


class _Fake:
    """A CPU callable as the model: nearest x``s`` plus a tenth of the tile's mean (so tiles differ from the whole frame); it records what it
    was given and what it returned."""

    def __init__(self, s):
        self.s, self.ins, self.outs = s, [], []

    def __call__(self, t):
        y = t.repeat_interleave(self.s, -1).repeat_interleave(self.s, -2) * 0.9 + t.float().mean().to(t.dtype) * 0.1
        self.ins.append(t)
        self.outs.append(y)
        return y


TILE, HALO = (12, 20), 8


def _native(m, h, w, s, tile, blend):
    """(f64 native frame of what the fake produced, extra error of the frame that was really written) of one call."""
    if tile is None:
        assert len(m.outs) == 1
        return m.outs[0].double(), 0.0
    tiles = plan_tiles(h, w, -(-h // tile[0]), -(-w // tile[1]), HALO)
    assert len(m.outs) == len(tiles) > 1
    native = TB.compose(tiles, m.outs, h, w, blend, s)
    return native, (2.0**-21 * max(1.0, native.abs().max().item()) if blend else 0.0)


@pytest.mark.parametrize('s', [2, 1])
@pytest.mark.parametrize('tile,blend', [(None, 0), (TILE, 0), (TILE, 4)])
@pytest.mark.parametrize('fmt,out_fmt,dtype', [('nv12', None, torch.float32), ('nv12', 'p010', torch.float32), ('p010', None, torch.float16), ('p010', 'nv12', torch.bfloat16)])
def test_upscale_yuv_with_a_cpu_callable(s, tile, blend, fmt, out_fmt, dtype):
    n, h, w = 2, 24, 40
    kw = dict(matrix='bt601', range='limited', chroma_loc='left')
    y, uv = Y.random_planes(n, h, w, fmt, seed=11)
    m = _Fake(s)
    gy, guv = resselt_amd.upscale_yuv(m, y, uv, fmt=fmt, out_fmt=out_fmt, tile=tile, halo=HALO, blend=blend, dtype=dtype, scale=s, **kw)
    what = f'fake x{s} {fmt}->{out_fmt or fmt} {dtype} tile {tile} blend {blend}'
    assert tuple(gy.shape) == (n, h * s, w * s) and tuple(guv.shape) == (n, h * s // 2, w * s // 2, 2)
    if tile is None:
        assert m.ins[0].dtype == dtype
        Y.assert_read(m.ins[0], y, uv, what, fmt=fmt, **kw)
    native, extra = _native(m, h, w, s, tile, blend)
    Y.assert_written(gy, guv, native, what, extra=extra, fmt=out_fmt or fmt, **kw)
    m1 = _Fake(s)  # [H, W] planes in, [H, W] planes out
    oy, ouv = resselt_amd.upscale_yuv(m1, y[0], uv[0], fmt=fmt, out_fmt=out_fmt, tile=tile, halo=HALO, blend=blend, dtype=dtype, scale=s, **kw)
    assert oy.dim() == 2 and ouv.dim() == 3 and tuple(oy.shape) == (h * s, w * s)


@pytest.mark.parametrize('tile,blend', [(None, 0), (TILE, 4)])
@pytest.mark.parametrize('okw,size', [(dict(out_size=(30, 52)), (30, 52)), (dict(out_scale=1.5), (36, 60)), (dict(out_size=(100, 90), resample='bilinear'), (100, 90))])
def test_upscale_yuv_out_size_resamples_before_the_one_rounding(tile, blend, okw, size):
    n, h, w, s = 1, 24, 40, 2
    kw = dict(matrix='bt2020', range='full', chroma_loc='center')
    y, uv = Y.random_planes(n, h, w, 'nv12', seed=12)
    m = _Fake(s)
    gy, guv = tiling.upscale_yuv(m, y, uv, out_fmt='p010', tile=tile, halo=HALO, blend=blend, dtype=torch.float32, scale=s, **kw, **okw)
    assert tuple(gy.shape) == (n, *size)
    native, extra = _native(m, h, w, s, tile, blend)
    filter = okw.get('resample', 'bicubic')
    ty, tx = resample_table(s * h, size[0], filter), resample_table(s * w, size[1], filter)
    extra = extra * R.abs_row_sum(ty) * R.abs_row_sum(tx) + R.bound(ty, tx, native.abs().max().item())
    Y.assert_written(gy, guv, R.interpolate64(native, size, filter), f'fake x2 nv12->p010 {okw} tile {tile} blend {blend}', extra=extra, fmt='p010', **kw)
    same = tiling.upscale_yuv(_Fake(s), y, uv, out_fmt='p010', tile=tile, halo=HALO, blend=blend, dtype=torch.float32, scale=s, out_size=(s * h, s * w), **kw)
    plain = tiling.upscale_yuv(_Fake(s), y, uv, out_fmt='p010', tile=tile, halo=HALO, blend=blend, dtype=torch.float32, scale=s, **kw)
    assert torch.equal(same[0], plain[0]) and torch.equal(same[1], plain[1])  # the native size changes nothing


class _Info:
    def __init__(self, cin, cout, upscale=2):
        self.in_channels, self.out_channels, self.upscale = cin, cout, upscale


class _WithInfo(_Fake):
    def __init__(self, cin, cout):
        super().__init__(2)
        self.parameters_info = _Info(cin, cout)


def test_refusals():
    y, uv = Y.random_planes(1, 24, 40, 'nv12', seed=1)
    up = tiling.upscale_yuv
    ran = _Fake(2)
    for bad in (dict(fmt='i420'), dict(out_fmt='yuy2'), dict(matrix='bt470'), dict(range='tv'), dict(chroma_loc='top'), dict(resample='lanczos')):
        with pytest.raises(ValueError, match=list(bad.values())[0]):
            up(ran, y, uv, scale=2, **bad)
    for cin, cout in ((1, 1), (4, 4), (3, 1), (1, 3)):
        with pytest.raises(ValueError, match='3 channels'):
            up(_WithInfo(cin, cout), y, uv)
    assert up(_WithInfo(3, 3), y, uv, dtype=torch.float32)[0].shape == (1, 48, 80)  # the scale comes from parameters_info
    with pytest.raises(ValueError, match='scale'):
        up(ran, y, uv)
    for by, buv in ((y[:, :23], uv), (y[:, :, :39], uv), (y[:, :22], uv), (y, uv[..., :1]), (y, uv[:, :, :19]), (y[0], uv), (y.to(torch.int32).to(torch.uint16), uv),
                    (y, uv.to(torch.int32).to(torch.uint16)), (y.float(), uv.float())):  # fmt: skip
        with pytest.raises(ValueError):
            up(ran, by, buv, scale=2)
    with pytest.raises(ValueError):
        up(ran, y, uv, fmt='p010', scale=2)  # uint8 planes are no P010
    for bad in (dict(out_size=(47, 80)), dict(out_size=(48, 81)), dict(out_scale=1.03)):  # 1.03: 25 x 41
        with pytest.raises(ValueError, match='odd'):
            up(ran, y, uv, scale=2, **bad)
    with pytest.raises(ValueError, match='not both'):
        up(ran, y, uv, scale=2, out_size=(10, 10), out_scale=2)
    with pytest.raises(ValueError, match='out_scale'):
        up(ran, y, uv, scale=2, out_scale=0)
    with pytest.raises(ValueError, match='out_size'):
        up(ran, y, uv, scale=2, out_size=(0, 10))
    with pytest.raises(ValueError, match='more than 8'):
        up(ran, y, uv, scale=2, out_size=(4, 80))
    with pytest.raises(ValueError, match='blend'):
        up(ran, y, uv, scale=2, blend=-1)
    assert not ran.ins  # every refusal came before the model ran
    with pytest.raises(ValueError, match='exceeds the halo'):
        up(ran, y, uv, scale=2, tile=TILE, halo=4, blend=6)
    with pytest.raises(ValueError):
        ops.nchw_to_yuv420(torch.zeros(1, 3, 5, 8))
    with pytest.raises(ValueError):
        ops.nchw_to_yuv420(torch.zeros(1, 4, 6, 8))
    with pytest.raises(TypeError):
        ops.yuv420_to_nchw(y, uv, dtype=torch.float64)
    assert 'upscale_yuv' in resselt_amd.__all__ and 'upscale' in resselt_amd.__all__


READ_ORDER = ['y', 'y_pitch', 'y_batch_stride', 'uv', 'uv_pitch', 'uv_batch_stride', 'bits', 'batch', 'H', 'W', 'matrix', 'full_range', 'chroma_loc', 'dst',
              'dst_dtype', 'stream']  # fmt: skip
WRITE_ORDER = ['src', 'src_dtype', 'batch', 'H', 'W', 'matrix', 'full_range', 'chroma_loc', 'bits', 'y', 'y_pitch', 'y_batch_stride', 'uv', 'uv_pitch',
               'uv_batch_stride', 'stream']  # fmt: skip


@pytest.mark.parametrize('name,order,flt', [('rsa_yuv420_to_nchw', READ_ORDER, 'dst'), ('rsa_nchw_to_yuv420', WRITE_ORDER, 'src')])
def test_internal_rows_name_the_arguments_in_the_order_of_the_documented_prototypes(name, order, flt):
    import os
    import re

    restype, params = L.INTERNAL[name]
    assert restype is C.c_int and [k for k, _ in params] == order
    for k, t in params:
        want = C.c_int64 if k.endswith(('_pitch', '_batch_stride')) else C.c_void_p if k in ('y', 'uv', flt, 'stream') else C.c_int32
        assert t is want, k
    assert name not in L.SIGNATURES and name not in L.EXTENSIONS  # no header declares it
    with open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), '..', 'csrc', 'yuv.hip')) as fh:
        text = fh.read()
    for where in (r'//\s+int ' + name, r'extern "C" int ' + name):  # the prototype in the head comment, and the definition
        proto = re.search(where + r'\(([^)]*)\)', text).group(1)
        assert [a.split()[-1].lstrip('*') for a in re.sub(r'\s*//\s*', ' ', proto).split(',')] == order, where


E_ARG, E_ALIGN = -1, -3
YP, UVP, FLT = 0x100000, 0x200000, 0x900000  # fake aligned addresses: every call below is refused before a launch


def _args(name, **over):
    a = dict(y=YP, y_pitch=64, y_batch_stride=64 * 32, uv=UVP, uv_pitch=64, uv_batch_stride=64 * 16, bits=8, batch=1, H=32, W=48, matrix=1, full_range=0,
             chroma_loc=0, stream=None)  # fmt: skip
    a.update({'dst': FLT, 'dst_dtype': L.F16} if name == 'rsa_yuv420_to_nchw' else {'src': FLT, 'src_dtype': L.F16})
    for k, v in over.items():
        a[{'flt': 'dst', 'flt_dtype': 'dst_dtype'}[k] if k.startswith('flt') and name == 'rsa_yuv420_to_nchw' else {'flt': 'src', 'flt_dtype': 'src_dtype'}.get(k, k)] = v
    return [a[k] for k, _ in L.INTERNAL[name][1]]


@pytest.mark.parametrize('name', ['rsa_yuv420_to_nchw', 'rsa_nchw_to_yuv420'])
@pytest.mark.parametrize('over,status', [
    (dict(y=None), E_ARG), (dict(uv=None), E_ARG), (dict(flt=None), E_ARG), (dict(bits=9), E_ARG), (dict(bits=12), E_ARG), (dict(bits=0), E_ARG),
    (dict(H=31), E_ARG), (dict(W=47), E_ARG), (dict(H=0), E_ARG), (dict(W=-2), E_ARG), (dict(batch=0), E_ARG),
    (dict(matrix=3), E_ARG), (dict(matrix=-1), E_ARG), (dict(full_range=2), E_ARG), (dict(chroma_loc=2), E_ARG), (dict(chroma_loc=-1), E_ARG),
    (dict(flt_dtype=3), E_ARG), (dict(flt_dtype=-1), E_ARG),
    (dict(y_pitch=47), E_ARG), (dict(uv_pitch=46), E_ARG), (dict(bits=10), E_ARG),  # P010 rows are 96 bytes: a pitch of 64 is too small
    (dict(batch=2, y_batch_stride=64 * 31), E_ARG), (dict(batch=2, uv_batch_stride=64 * 15), E_ARG),
    (dict(H=16 * 65535 + 2), E_ARG), (dict(batch=65536), E_ARG),  # the grid
    (dict(bits=10, y_pitch=128, uv_pitch=128, y=YP + 1), E_ALIGN), (dict(bits=10, y_pitch=129, uv_pitch=128), E_ALIGN),
    (dict(bits=10, y_pitch=128, uv_pitch=128, batch=2, y_batch_stride=128 * 32 + 1, uv_batch_stride=128 * 16), E_ALIGN),
    (dict(uv=UVP + 1), E_ALIGN), (dict(uv_pitch=65), E_ALIGN), (dict(batch=2, uv_batch_stride=64 * 16 + 1), E_ALIGN),
    (dict(bits=10, y_pitch=128, uv_pitch=128, uv=UVP + 2), E_ALIGN), (dict(bits=10, y_pitch=128, uv_pitch=130), E_ALIGN),
    (dict(flt=FLT + 1), E_ALIGN), (dict(flt=FLT + 2, flt_dtype=L.F32), E_ALIGN), (dict(flt=FLT + 1, flt_dtype=L.BF16), E_ALIGN),
])  # fmt: skip
def test_argument_checks_return_before_any_launch(name, over, status):
    lib = L.load()
    assert getattr(lib, name)(*_args(name, **over)) == status, over
    assert name.encode() in lib.rsa_last_error_string()
