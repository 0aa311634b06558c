"""Any output size end to end on the GPU: ``resselt_amd.upscale(out_size= / out_scale=)`` and ``upscale_tiled`` with synth checkpoints.

The expected value is always torch's f64 antialiased interpolation (tests/resample_reference.py) of the SAME engine model's own native
frame -- ``m(x)``, or ``tile_blend_reference.compose`` of its tile outputs (``blend = 0``: the hard crop) -- never the code under test's
own resampling.  Float results: within ``B = (T_h + T_w + 4) * 2^-24 * S_h * S_w * max(1, |y|max)`` from the call's tables, plus one rounding
of the returned dtype.  8-bit results: within ``0.5 + 255 * B`` of ``255 * clamp(v64, 0, 1)``.  Where the native frame is the f32 sum of a
blend, ``2^-21 * S_h * S_w * max(1, |y|max)`` is added for that sum (tests/test_tile_blend_kernels_gpu.py derives it)."""

import pytest
import torch

import resample_reference as R
import resselt_amd
import tile_blend_reference as TB
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.tiling import resample_table
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

TILE, HALO = (20, 28), 8
ROUNDING = {torch.float32: 2.0**-24, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _plan(h, w):
    return tiling.plan_tiles(h, w, -(-h // TILE[0]), -(-w // TILE[1]), HALO)


def _tile_outputs(m, x, tiles):
    """What the model makes of every tile's read window, as f64 [N, C, h, w] on the CPU (8-bit outputs as code / 255)."""
    outs = []
    for t in tiles:
        crop = (x[:, t.ry0 : t.ry1, t.rx0 : t.rx1] if x.dtype == torch.uint8 else x[:, :, t.ry0 : t.ry1, t.rx0 : t.rx1]).contiguous()
        y = m(crop).cpu()
        outs.append(R.image_as_f64(y) if y.dtype == torch.uint8 else y.double())
    return outs


def _image(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def _bound(native, size, filter, blended=False):
    """B of resampling the f64 ``native`` frame [N, C, H, W] to ``size`` (plus the f32 blend sum's own error)."""
    ty, tx = resample_table(native.shape[2], size[0], filter), resample_table(native.shape[3], size[1], filter)
    xmax = native.abs().max().item()
    return R.bound(ty, tx, xmax) + (2.0**-21 * R.abs_row_sum(ty) * R.abs_row_sum(tx) * max(1.0, xmax) if blended else 0.0)


def check_image(got, native, size, filter, what, blended=False):
    want = R.interpolate64(native, size, filter)
    b = _bound(native, size, filter, blended)
    got = got.cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (native.shape[0], *size, native.shape[1]), what
    err = R.image_error(got, want)
    print(f'MEASURE {what}: {err:.5f} codes, (error - 0.5) / (255 B) = {(err - 0.5) / (255 * b):.3f}')
    assert err <= 0.5 + 255 * b, what


def check_float(got, native, size, filter, what, blended=False):
    want = R.interpolate64(native, size, filter)
    b = _bound(native, size, filter, blended)
    assert tuple(got.shape) == tuple(want.shape), what
    over = (got.cpu().double() - want).abs() - (ROUNDING[got.dtype] * want.abs() + 2.0**-25)
    print(f'MEASURE {what}: worst error beyond the rounding of {got.dtype} {over.max().item() / b:.3f} of B = {b:.2e}')
    assert bool((over <= b).all()), what


def _compact(device, seed=7):
    return resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=32, num_conv=3, upscale=4, seed=seed))).to(device)


def _size(h, w, out_scale):
    import math

    return max(1, math.floor(h * out_scale + 0.5)), max(1, math.floor(w * out_scale + 0.5))


@pytest.mark.parametrize('h,w,n', [(40, 56, 1), (36, 52, 2)])
@pytest.mark.parametrize('out_scale', [2, 3, 2.5])
def test_compact_untiled(device, out_scale, h, w, n):
    m = _compact(device)
    img = _image(n, h, w, seed=3).to(device)
    for dtype in (torch.float16, torch.float32):
        x = ops.image_u8_to_nchw(img, dtype)
        y0 = m(x)
        native = y0.cpu().double()
        launches = m.launches_per_forward()
        size = _size(h, w, out_scale)
        image = img if n > 1 else img[0]
        got = resselt_amd.upscale(m, image, dtype=dtype, out_scale=out_scale)
        assert got.dim() == image.dim()
        check_image(got if n > 1 else got[None], native, size, 'bicubic', f'compact x4 {dtype} untiled {h}x{w} N={n} out_scale {out_scale}')
        assert torch.equal(resselt_amd.upscale(m, image, dtype=dtype, out_size=size), got)  # the same size spelled as out_size
        y = tiling.upscale_tiled(m, x, 4, tile=(64, 64), out_scale=out_scale, resample='bilinear')  # fits one tile; the model's dtype comes back
        assert y.dtype == y0.dtype
        check_float(y, native, size, 'bilinear', f'compact x4 {dtype} upscale_tiled one tile {h}x{w} N={n} out_scale {out_scale} bilinear')
        assert launches is not None and m.launches_per_forward() == launches  # the model ran on the same plan: out_scale is not its business


@pytest.mark.parametrize('h,w,n', [(40, 56, 2), (36, 52, 1)])
@pytest.mark.parametrize('blend', [0, 4])
def test_compact_tiles(device, blend, h, w, n):
    """Hard-crop tiles (``blend = 0``) and the f32 sum of a blend as the frame that is resampled."""
    m = _compact(device)
    img = _image(n, h, w, seed=4).to(device)
    tiles = _plan(h, w)
    assert len(tiles) == 4
    for dtype, kw, size in ((torch.float16, dict(out_scale=2), (2 * h, 2 * w)), (torch.float32, dict(out_size=(3 * h + 1, 5 * w)), (3 * h + 1, 5 * w))):
        x = ops.image_u8_to_nchw(img, dtype)
        native = TB.compose(tiles, _tile_outputs(m, x, tiles), h, w, blend, 4)
        what = f'compact x4 {dtype} tiles blend {blend} {h}x{w} N={n} {kw}'
        got = resselt_amd.upscale(m, img, tile=TILE, halo=HALO, dtype=dtype, blend=blend, **kw)
        check_image(got, native, size, 'bicubic', what, blended=blend > 0)
        y = tiling.upscale_tiled(m, x, 4, tile=TILE, halo=HALO, blend=blend, **kw)
        assert y.dtype == tiling.upscale_tiled(m, x, 4, tile=TILE, halo=HALO, blend=blend).dtype
        check_float(y, native, size, 'bicubic', what + ' upscale_tiled', blended=blend > 0)


def _u8_models(device):
    return {
        'rrdbnet': (resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=1, scale=4, seed=9))).to(device), 4),
        'rcan': (resselt_amd.load_from_state_dict(dict(synth.rcan_state_dict(scale=2, n_resgroups=2, n_resblocks=2, seed=31))).to(device), 2),
    }


@pytest.mark.parametrize('h,w,n', [(40, 56, 1), (36, 52, 2)])
@pytest.mark.parametrize('tiled', [False, True])
def test_rrdbnet_8_bit_in_and_out(device, tiled, h, w, n):
    m, s = _u8_models(device)['rrdbnet']
    assert m.supports_u8
    img = _image(n, h, w, seed=5).to(device)
    m(img)
    launches = m.launches_per_forward()
    for kw, size, filter in ((dict(out_scale=2), (2 * h, 2 * w), 'bicubic'), (dict(out_scale=3), (3 * h, 3 * w), 'bilinear'), (dict(out_scale=2.5), _size(h, w, 2.5), 'bicubic')):
        what = f'rrdbnet x4 8-bit {"blend 4" if tiled else "untiled"} {h}x{w} N={n} {kw} {filter}'
        if tiled:
            tiles = _plan(h, w)
            native = TB.compose(tiles, _tile_outputs(m, img, tiles), h, w, 4, s)
            got = resselt_amd.upscale(m, img, tile=TILE, halo=HALO, blend=4, resample=filter, **kw)
        else:
            native = R.image_as_f64(m(img).cpu())
            got = resselt_amd.upscale(m, img, resample=filter, **kw)
        check_image(got, native, size, filter, what, blended=tiled)
        if not tiled:
            assert launches is not None and m.launches_per_forward() == launches


@pytest.mark.parametrize('h,w,n', [(40, 56, 2), (36, 52, 1)])
def test_rcan_x2_delivers_x1(device, h, w, n):
    m, s = _u8_models(device)['rcan']
    img = _image(n, h, w, seed=6).to(device)
    native = R.image_as_f64(m(img).cpu())
    assert tuple(native.shape) == (n, 3, 2 * h, 2 * w)
    check_image(resselt_amd.upscale(m, img, out_size=(h, w)), native, (h, w), 'bicubic', f'rcan x2 8-bit at x1 {h}x{w} N={n}')
    hard = TB.compose(_plan(h, w), _tile_outputs(m, img, _plan(h, w)), h, w, 0, s)
    check_image(resselt_amd.upscale(m, img, tile=TILE, halo=HALO, out_size=(h, w)), hard, (h, w), 'bicubic', f'rcan x2 8-bit hard crop at x1 {h}x{w} N={n}')


def test_native_size_is_the_plain_call(device):
    h, w = 40, 56
    img = _image(2, h, w, seed=8).to(device)
    m = _compact(device)
    for kw in (dict(), dict(tile=TILE, halo=HALO), dict(tile=TILE, halo=HALO, blend=4)):
        plain = resselt_amd.upscale(m, img, **kw)
        assert torch.equal(resselt_amd.upscale(m, img, out_size=(4 * h, 4 * w), **kw), plain)
        assert torch.equal(resselt_amd.upscale(m, img, out_scale=4, resample='bilinear', **kw), plain)
    x = ops.image_u8_to_nchw(img, torch.float16)
    assert torch.equal(tiling.upscale_tiled(m, x, 4, tile=TILE, halo=HALO, out_scale=4.0), tiling.upscale_tiled(m, x, 4, tile=TILE, halo=HALO))
    r, s = _u8_models(device)['rrdbnet']
    for kw in (dict(), dict(tile=TILE, halo=HALO), dict(tile=TILE, halo=HALO, blend=4)):
        assert torch.equal(resselt_amd.upscale(r, img, out_size=(s * h, s * w), **kw), resselt_amd.upscale(r, img, **kw))
    with pytest.raises(ValueError, match='more than 8'):
        resselt_amd.upscale(m, img, out_size=(4 * h, 27))
    with pytest.raises(ValueError, match='not both'):
        resselt_amd.upscale(m, img, out_size=(10, 10), out_scale=2)
