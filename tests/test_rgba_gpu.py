"""``resselt_amd.upscale_rgba`` end to end on the GPU with synth checkpoints: a Compact x2 (no ``supports_u8``) and an RRDBNet (``nb = 1``)
x4, which has ``supports_u8`` and takes the float path here like every model.

The model is wrapped so that every call records its input and its output.  The recorded input must be within the read bound of the f64 read +
bleed definition of the image (of the tile's read window, where the frame is tiled); the returned image must be within the write bound of the
f64 write definition applied to the frame the recorded outputs make: the output itself, ``tile_blend_reference.compose`` of the tiles' outputs,
or torch's f64 antialiased interpolation of either (``out_scale``).  With ``alpha='resample'`` the alpha target is the f64 interpolation of the
image's alpha.  Nothing expected comes from the code under test.  Bounds: tests/rgba_reference.py; the f32 blend sum adds
``2^-21 * max(1, |y|max)`` and the f32 resampling its own bound (tests/resample_reference.py), both times ``M``."""

import pytest
import torch

import resample_reference as R
import resselt_amd
import rgba_reference as G
import tile_blend_reference as TB
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.tiling import resample_table
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

H, W, TILE, HALO, BLEED = 48, 64, (24, 32), 8, 8


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


_MODELS: dict = {}


def _models(device):
    """name -> (model, scale), made once for all tests of this file."""
    if not _MODELS:
        _MODELS['compact'] = (resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=32, num_conv=3, upscale=2, seed=7))).to(device), 2)
        _MODELS['rrdbnet'] = (resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=1, scale=4, seed=9))).to(device), 4)
    return _MODELS


def _image(n, c, bits, opaque=False, seed=31):
    img = G.random_image(n, H, W, c, bits, seed=seed + n, transparent=0.6)
    return G.with_alpha(img, G.DEPTHS[bits][1]) if (opaque and G.has_alpha(c)) else img


def _run(device, name, c=4, bits=8, n=1, alpha='model', opaque=False, dtype=torch.float16, **call):
    """One ``upscale_rgba`` call checked end to end; returns the image."""
    model, s = _models(device)[name]
    assert not getattr(model, 'supports_u8', False) or name == 'rrdbnet'
    img = _image(n, c, bits, opaque)
    out_bits = call.get('out_bits') or bits
    m = Recorded(model)
    got = resselt_amd.upscale_rgba(m, img.to(device), alpha=alpha, bleed=BLEED, dtype=dtype, **call)
    what = f'{name} x{s} C={c} {bits}->{out_bits} {dtype} N={n} {alpha} opaque={opaque} {call}'
    translucent = G.has_alpha(c) and not opaque
    batch = 2 * n if (translucent and alpha == 'model') else n
    tile, blend = call.get('tile'), call.get('blend', 0)
    want_in = G.model_input64(img, 3, alpha, BLEED)
    assert want_in.shape[0] == batch
    if tile is None:
        assert len(m.ins) == 1 and m.ins[0].dtype == dtype  # one call: alpha rides in the same batch
        G.assert_read(m.ins[0], img, 3, alpha, BLEED, what)
        native, extra = m.outs[0].cpu().double(), 0.0
    else:
        tiles = tiling.plan_tiles(H, W, -(-H // tile[0]), -(-W // tile[1]), call.get('halo', 32))
        assert len(m.ins) == len(tiles) == 4  # the model runs once per tile
        for t, x in zip(tiles, m.ins):
            crop = want_in[:, :, t.ry0 : t.ry1, t.rx0 : t.rx1]
            assert tuple(x.shape) == tuple(crop.shape) and bool(((x.cpu().double() - crop).abs() <= G.read_bound(dtype, crop, BLEED)).all()), f'{what}: tile {t.index} input'
        native = TB.compose(tiles, [o.cpu() for o in m.outs], H, W, blend, s)
        extra = 2.0**-21 * max(1.0, native.abs().max().item()) if blend else 0.0
    assert native.shape[0] == batch, what
    size = (H * s, W * s)
    if 'out_scale' in call:
        size = (int(H * call['out_scale']), int(W * call['out_scale']))
        ty, tx = resample_table(s * H, size[0], 'bicubic'), resample_table(s * W, size[1], 'bicubic')
        extra = extra * R.abs_row_sum(ty) * R.abs_row_sum(tx) + R.bound(ty, tx, native.abs().max().item())
        native = R.interpolate64(native, size, 'bicubic')
    assert got.is_cuda and tuple(got.shape) == (n, *size, c) and got.dtype == G.DEPTHS[out_bits][0], what
    got = got.cpu()
    if not G.has_alpha(c):
        G.assert_written(got, native, None, what, extra=extra)
    elif not translucent:  # the opaque shortcut: the model saw N entries, alpha is the maximum code
        G.assert_written(got, native, None, what, extra=extra)
        assert set(got[..., c - 1].to(torch.int32).flatten().tolist()) == {G.DEPTHS[out_bits][1]}, what
    elif alpha == 'model':
        G.assert_written(got, native[:n], native[n:], what, extra=extra)
    else:
        G.assert_written(got[..., : c - 1].contiguous(), native, None, what + ' colour', extra=extra)
        a64 = G.read64(img, BLEED)[1]
        ty, tx = resample_table(H, size[0], 'bicubic'), resample_table(W, size[1], 'bicubic')
        target = (R.interpolate64(a64, size, 'bicubic').clamp(0, 1) * G.DEPTHS[out_bits][1]).permute(0, 2, 3, 1)
        err = G.code_error(got[..., c - 1 :].contiguous(), target)
        assert err <= G.write_bound(out_bits, R.bound(ty, tx, 1.0) + G.U), f'{what}: alpha {err:.5f} codes'
    return got


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
@pytest.mark.parametrize('alpha', ['model', 'resample'])
def test_whole_frame(device, name, alpha):
    _run(device, name, alpha=alpha)
    _run(device, name, bits=16, alpha=alpha, dtype=torch.float32)


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
@pytest.mark.parametrize('alpha', ['model', 'resample'])
def test_the_opaque_shortcut(device, name, alpha):
    _run(device, name, alpha=alpha, opaque=True, n=2)
    _run(device, name, c=2, alpha=alpha, opaque=True)


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
@pytest.mark.parametrize('alpha', ['model', 'resample'])
def test_tiles_with_blend(device, name, alpha):
    _run(device, name, alpha=alpha, tile=TILE, halo=HALO, blend=4)


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
@pytest.mark.parametrize('alpha', ['model', 'resample'])
def test_out_scale(device, name, alpha):
    _run(device, name, alpha=alpha, out_scale=1.5)
    _run(device, name, alpha=alpha, tile=TILE, halo=HALO, blend=4, out_scale=1.5, dtype=torch.float32)


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
def test_an_8_bit_source_is_delivered_in_16_bits(device, name):
    got = _run(device, name, out_bits=16, dtype=torch.float32)
    assert got.dtype == torch.uint16
    _run(device, name, bits=16, out_bits=8, n=2, alpha='resample')


@pytest.mark.parametrize('name', ['compact', 'rrdbnet'])
def test_gray_and_gray_with_alpha_on_a_three_channel_model(device, name):
    _run(device, name, c=1)
    _run(device, name, c=2, bits=16, dtype=torch.float32)
    _run(device, name, c=2, alpha='resample', tile=TILE, halo=HALO, blend=4)
    _run(device, name, c=3, bits=16, n=2)


def test_uint8_rgb_equals_upscale_bit_for_bit_and_upscale_is_unchanged(device):
    model, s = _models(device)['compact']
    img = _image(2, 3, 8).to(device)
    for call in (dict(), dict(tile=TILE, halo=HALO, blend=4), dict(tile=TILE, halo=HALO), dict(out_scale=1.5), dict(tile=TILE, halo=HALO, blend=4, out_size=(50, 70))):
        before = resselt_amd.upscale(model, img, **call)
        got = resselt_amd.upscale_rgba(model, img, **call)
        after = resselt_amd.upscale(model, img, **call)
        assert got.dtype == torch.uint8 and torch.equal(got, before), f'{call}: upscale_rgba differs from upscale in {int((got != before).sum())} codes'
        assert torch.equal(before, after), call
    one = resselt_amd.upscale_rgba(model, img[0])
    assert one.dim() == 3 and torch.equal(one, resselt_amd.upscale(model, img[0]))
    rgba = torch.cat((img, torch.full_like(img[..., :1], 255)), -1)  # opaque RGBA: the RGB result plus the maximum alpha
    got = resselt_amd.upscale_rgba(model, rgba)
    assert torch.equal(got[..., :3], resselt_amd.upscale(model, img)) and bool((got[..., 3] == 255).all())
