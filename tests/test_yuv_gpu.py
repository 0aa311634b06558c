"""``resselt_amd.upscale_yuv`` end to end on the GPU with synth checkpoints: a Compact x2 and an RRDBNet (``nb = 1``) x4, which has
``supports_u8`` and takes the float path here like every model.

The model is wrapped so that every call records its input and its output.  The recorded input must be within the read bound of the f64
``to_rgb64`` of the planes (of the tile's read window, where the frame is tiled); the returned planes must be within the write bound of the f64
``to_yuv64`` of the frame the recorded outputs make: the output itself, ``tile_blend_reference.compose`` of the tiles' outputs (``blend = 0``:
the hard crop), or torch's f64 antialiased interpolation of either (``out_scale``).  Nothing expected comes from the code under test.
Bounds: tests/yuv_reference.py; the f32 blend sum adds ``2^-21 * max(1, |y|max)`` and the f32 resampling its own bound
(tests/resample_reference.py), both times 2^bits."""

import pytest
import torch

import resample_reference as R
import resselt_amd
import tile_blend_reference as TB
import yuv_reference as Y
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.tiling import resample_table
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

H, W, TILE, HALO = 24, 40, (12, 20), 8


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


class Recorded:
    """The model with its attributes (``parameters_info``, ``supports_u8``), recording a copy of what each call was given and returned."""

    def __init__(self, model):
        self._model, self.ins, self.outs = model, [], []

    def __getattr__(self, name):
        return getattr(self._model, name)

    def __call__(self, x):
        y = self._model(x)
        self.ins.append(x.detach().clone())
        self.outs.append(y.detach().clone())
        return y


def _models(device):
    return {
        'compact': (resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=32, num_conv=3, upscale=2, seed=7))).to(device), 2),
        'rrdbnet': (resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=1, scale=4, seed=9))).to(device), 4),
    }


def _run(device, name, n=1, fmt='nv12', dtype=torch.float16, kw=None, **call):
    """One ``upscale_yuv`` call checked end to end; returns the planes."""
    model, s = _models(device)[name]
    kw = kw or dict(matrix='bt709', range='limited', chroma_loc='left')
    out_fmt = call.get('out_fmt') or fmt
    y, uv = Y.random_planes(n, H, W, fmt, seed=31 + n)
    m = Recorded(model)
    gy, guv = resselt_amd.upscale_yuv(m, y.to(device), uv.to(device), fmt=fmt, dtype=dtype, **kw, **call)
    what = f'{name} x{s} {fmt}->{out_fmt} {dtype} N={n} {call}'
    tile, blend = call.get('tile'), call.get('blend', 0)
    want_in = Y.to_rgb64(y, uv, fmt, **kw)
    if tile is None:
        assert len(m.ins) == 1 and m.ins[0].dtype == dtype
        Y.assert_read(m.ins[0], y, uv, what, fmt=fmt, **kw)
        native, extra = m.outs[0].cpu().double(), 0.0
    else:
        tiles = tiling.plan_tiles(H, W, -(-H // tile[0]), -(-W // tile[1]), call.get('halo', 32))
        assert len(m.ins) == len(tiles) == 4
        for t, got in zip(tiles, m.ins):  # every tile read its window of the converted frame
            crop = want_in[:, :, t.ry0 : t.ry1, t.rx0 : t.rx1]
            assert bool(((got.cpu().double() - crop).abs() <= Y.read_bound(dtype, crop)).all()), f'{what}: tile {t.index} input'
        native = TB.compose(tiles, [o.cpu() for o in m.outs], H, W, blend, s)
        extra = 2.0**-21 * max(1.0, native.abs().max().item()) if blend else 0.0
    size = (H * s, W * s)
    if 'out_scale' in call:
        size = (int(H * call['out_scale']), int(W * call['out_scale']))
        ty, tx = resample_table(s * H, size[0], 'bicubic'), resample_table(s * W, size[1], 'bicubic')
        extra = extra * R.abs_row_sum(ty) * R.abs_row_sum(tx) + R.bound(ty, tx, native.abs().max().item())
        native = R.interpolate64(native, size, 'bicubic')
    assert gy.is_cuda and tuple(gy.shape) == (n, *size) and tuple(guv.shape) == (n, size[0] // 2, size[1] // 2, 2), what
    Y.assert_written(gy, guv, native, what, extra=extra, fmt=out_fmt, **kw)
    return gy, guv


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
def test_whole_frame(device, name):
    _run(device, name)
    _run(device, name, fmt='p010', dtype=torch.float32, kw=dict(matrix='bt2020', range='full', chroma_loc='center'))


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
@pytest.mark.parametrize('blend', [0, 4])
def test_tiles(device, name, blend):
    _run(device, name, tile=TILE, halo=HALO, blend=blend)


@pytest.mark.parametrize('name,out_scale', [('compact', 1.5), ('rrdbnet', 2), ('rrdbnet', 2.5)])
def test_out_scale_below_the_scale_of_the_model(device, name, out_scale):
    _run(device, name, out_scale=out_scale)
    _run(device, name, tile=TILE, halo=HALO, blend=4, out_scale=out_scale, dtype=torch.float32)


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
def test_an_8_bit_source_is_delivered_in_10_bits(device, name):
    gy, _ = _run(device, name, out_fmt='p010', dtype=torch.float32)
    assert gy.dtype == torch.uint16
    _run(device, name, out_fmt='p010', tile=TILE, halo=HALO, blend=4)


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
def test_batch_of_two_and_single_planes(device, name):
    _run(device, name, n=2)
    _run(device, name, n=2, tile=TILE, halo=HALO, blend=4, out_fmt='p010')
    model, s = _models(device)[name]
    y, uv = Y.random_planes(2, H, W, 'nv12', seed=33)
    oy, ouv = resselt_amd.upscale_yuv(model, y[1].to(device), uv[1].to(device))  # [H, W] planes in, [H, W] planes out
    assert tuple(oy.shape) == (H * s, W * s) and tuple(ouv.shape) == (H * s // 2, W * s // 2, 2) and oy.dtype == torch.uint8
    with pytest.raises(ValueError, match='odd'):
        resselt_amd.upscale_yuv(model, y.to(device), uv.to(device), out_size=(H * s - 1, W * s))
