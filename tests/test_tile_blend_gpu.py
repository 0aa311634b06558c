"""Seam blending end to end on the GPU: ``resselt_amd.upscale(blend=)`` and ``upscale_tiled(blend=)`` with synth checkpoints.

The expected value is always the f64 blend (tests/tile_blend_reference.py) of the SAME engine model's per-tile outputs ``m(crop)``, never the
code under test's own blend.  Float tensors: max-abs <= 2^-21 * max(1, |y|max) (test_tile_blend_kernels_gpu.py derives the bound).  8-bit
images: pixels outside all bands equal the hard crop bit for bit; a band pixel equals the f64 value rounded half to even, except that a pixel
whose f64 value lies within 1e-3 of a tie may differ by one code, and at most 1 % of the band pixels may be that close to a tie.  The seeds
below were checked with the CPU oracles of the same checkpoints on the same tiles: 0.17 % to 0.23 % of Compact's band values are within
1e-3 of a tie, and none of RRDBNet's and RCAN's (their 8-bit tiles differ by a code or two, and a weighted sum of two such codes with
weights (2i + 1) / (4 * blend * scale) cannot land on a half)."""

import pytest
import torch

import resselt_amd
import tile_blend_reference as R
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

TOL = 2.0**-21
SMOSR_REL = 2e-4  # test_smosr_gpu.py: hard-crop tiling against untiled, max-abs <= 2e-4 * max(1, |y|max)


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _plan(h, w, tile, halo, align=1):
    return tiling.plan_tiles(h, w, -(-h // tile[0]), -(-w // tile[1]), halo, align)


def _tile_outputs(m, x, tiles):
    """What the model makes of every tile's read window, as f64 [N, C, h, w] on the CPU (8-bit outputs as code / 255)."""
    outs = []
    for t in tiles:
        crop = (x[:, t.ry0 : t.ry1, t.rx0 : t.rx1] if x.dtype == torch.uint8 else x[:, :, t.ry0 : t.ry1, t.rx0 : t.rx1]).contiguous()
        y = m(crop).cpu()
        outs.append(R.image_as_f64(y) if y.dtype == torch.uint8 else y.double())
    return outs


def _two_halves_image(n, h, w, seed):
    """uint8 [N, H, W, 3]: noise around a dark left half and a bright right half."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, h, w, 3), generator=g) * 0.25 + 0.1
    x[:, :, w // 2 :] += 0.5
    return (x * 255).round().to(torch.uint8)


def check_u8(got, want01, band, hard, what):
    """``got`` / ``hard``: uint8 [N, H, W, C] with and without blending; ``want01``: the f64 blend [N, C, H, W] on the 0..1 scale."""
    got, hard = got.cpu().permute(0, 3, 1, 2), hard.cpu().permute(0, 3, 1, 2)
    assert got.dtype == torch.uint8 and got.shape == want01.shape == hard.shape, what
    assert torch.equal(got[..., ~band], hard[..., ~band]), f'{what}: a pixel outside the bands differs from the hard crop'
    v = (want01.clamp(0, 1) * 255)[..., band]
    g = got.double()[..., band]
    tie = ((v - v.floor()) - 0.5).abs() <= 1e-3
    share = tie.double().mean().item()
    off = (g - v.round()).abs()
    print(f'MEASURE {what}: {int(band.sum())} band pixels, {100 * share:.3f} % within 1e-3 of a tie, {int((off > 0).sum())} values off the rounded f64 value')
    assert share <= 0.01, f'{what}: {share:.4f} of the band pixels are near a tie'
    assert bool((off[~tie] == 0).all()) and bool((off[tie] <= 1).all()), f'{what}: {int((off[~tie] > 0).sum())} band values differ from the f64 blend'


def _compact(device, seed=7):
    return resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=32, num_conv=3, upscale=4, seed=seed))).to(device)


@pytest.mark.parametrize('h,w,tile,blend,n', [(40, 56, (20, 28), 4, 1), (40, 56, (20, 28), 1, 2), (36, 52, (20, 28), 4, 2), (40, 56, (40, 19), 4, 1)])
def test_float_tensors_match_the_f64_blend_of_the_tiles(device, h, w, tile, blend, n):
    m = _compact(device)
    x = synth.synth_input((n, 3, h, w), seed=40 + blend).to(device)
    tiles = _plan(h, w, tile, 8)
    assert len(tiles) == (3 if tile[0] == 40 else 4)
    want = R.compose(tiles, _tile_outputs(m, x, tiles), h, w, blend, 4)
    y = tiling.upscale_tiled(m, x, 4, tile=tile, halo=8, blend=blend)
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, 3, 4 * h, 4 * w)
    err = (y.cpu().double() - want).abs().max().item()
    print(f'MEASURE compact x4 {h}x{w} tile {tile} blend {blend} N={n}: max-abs {err:.3e} (|y|max {want.abs().max():.3f})')
    assert err <= TOL * max(1.0, want.abs().max().item())
    band = R.band_mask(tiles, h, w, blend, 4)
    hard = tiling.upscale_tiled(m, x, 4, tile=tile, halo=8)
    assert torch.equal(y.cpu()[..., ~band], hard.cpu()[..., ~band]) and not torch.equal(y, hard)
    assert torch.equal(tiling.upscale_tiled(m, x, 4, tile=tile, halo=8, blend=blend), y)  # bit-identical from run to run
    assert torch.equal(tiling.upscale_tiled(m, x, 4, tile=(h, w), halo=8, blend=blend), m(x))  # one tile: untiled


@pytest.mark.parametrize('dtype,blend,n', [(torch.float32, 4, 2), (torch.float16, 1, 1), (torch.float16, 4, 1)])
def test_uint8_images_through_a_float_model(device, dtype, blend, n):
    """Compact writes float tensors: its tiles are blended from ``dtype`` sources and the f32 sum is rounded to 8 bits once."""
    m = _compact(device)
    h, w, tile = 40, 56, (20, 28)
    img = _two_halves_image(n, h, w, seed=3).to(device)
    tiles = _plan(h, w, tile, 8)
    want = R.compose(tiles, _tile_outputs(m, ops.image_u8_to_nchw(img, dtype), tiles), h, w, blend, 4)
    image = img if n > 1 else img[0]
    got, hard = resselt_amd.upscale(m, image, tile=tile, halo=8, dtype=dtype, blend=blend), resselt_amd.upscale(m, image, tile=tile, halo=8, dtype=dtype)
    assert got.dim() == image.dim()
    got, hard = (got, hard) if n > 1 else (got[None], hard[None])
    check_u8(got, want, R.band_mask(tiles, h, w, blend, 4), hard, f'compact x4 {dtype} blend {blend} N={n}')
    assert torch.equal(resselt_amd.upscale(m, image, tile=(64, 64), halo=8, dtype=dtype, blend=blend), resselt_amd.upscale(m, image, dtype=dtype))


def _u8_models(device):
    return {
        'rrdbnet': (resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=1, scale=4, seed=9))).to(device), 4),
        'rcan': (resselt_amd.load_from_state_dict(dict(synth.rcan_state_dict(scale=2, n_resgroups=2, n_resblocks=2, seed=31))).to(device), 2),
    }


@pytest.mark.parametrize('h,w,tile,blend,n', [(40, 56, (20, 28), 4, 1), (36, 52, (20, 28), 1, 2), (40, 56, (40, 19), 4, 2)])
@pytest.mark.parametrize('name', ['rrdbnet', 'rcan'])
def test_uint8_images_through_models_that_write_8_bit_tiles(device, name, h, w, tile, blend, n):
    """RRDBNet and RCAN (whole-image pooling: its tiles do differ) write uint8 NHWC tiles: the kernel's 8-bit source."""
    m, s = _u8_models(device)[name]
    assert m.supports_u8
    img = _two_halves_image(n, h, w, seed=5).to(device)
    tiles = _plan(h, w, tile, 8)
    want = R.compose(tiles, _tile_outputs(m, img, tiles), h, w, blend, s)
    got = resselt_amd.upscale(m, img, tile=tile, halo=8, blend=blend)
    hard = resselt_amd.upscale(m, img, tile=tile, halo=8)
    check_u8(got, want, R.band_mask(tiles, h, w, blend, s), hard, f'{name} x{s} {h}x{w} tile {tile} blend {blend} N={n}')
    assert torch.equal(resselt_amd.upscale(m, img, tile=(64, 64), halo=8, blend=blend), resselt_amd.upscale(m, img))  # one tile: untiled


def test_exact_halo_model_blends_to_the_untiled_image(device):
    """SMoSR's reach (22 pixels) is inside the halo of 32: tiles agree inside the bands and the blend changes nothing beyond rounding.
    Tile (16, 24), halo 32, blend 8 as in test_smosr_gpu.py's tiled test -- on 48 x 48, where the three rows of tiles are 16 high: on
    that test's 40 x 40 the rows are 13, 14 and 13 high, 2 * blend = 16 does not fit and is refused; there the largest blend, 6, runs."""
    sd = synth.smosr_state_dict(seed=31, head_gain=4.0)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    for size, blend in ((48, 8), (40, 6)):
        x = synth.synth_input((1, 3, size, size), 31).to(device)
        img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
        full = tiling.upscale(m, img, dtype=torch.float32)
        tiled = tiling.upscale(m, img, tile=(16, 24), halo=32, dtype=torch.float32, blend=blend)
        assert tiled.shape == full.shape == (2 * size, 2 * size, 3) and tiled.dtype == torch.uint8
        assert (tiled.int() - full.int()).abs().max().item() <= 1
        yf = m(x)
        yt = tiling.upscale_tiled(m, x, 2, tile=(16, 24), halo=32, blend=blend)
        err = (yt - yf).abs().max().item()
        print(f'MEASURE smosr {size}x{size} blend {blend} against untiled: {err:.3e}')
        assert yt.dtype == yf.dtype and err <= SMOSR_REL * max(1.0, yf.abs().max().item())
    with pytest.raises(ValueError, match=r'2 \* blend = 16 exceeds the tile extent of 13'):
        tiling.upscale_tiled(m, x, 2, tile=(16, 24), halo=32, blend=8)


def _seam_jump(d, tiles, s):
    """Largest mean absolute jump of ``d`` [N, C, H, W] across a seam line (an interior tile edge, in output pixels)."""
    rows = sorted({t.y0 * s for t in tiles if t.y0 > 0})
    cols = sorted({t.x0 * s for t in tiles if t.x0 > 0})
    jumps = [(d[:, :, r] - d[:, :, r - 1]).abs().mean().item() for r in rows] + [(d[:, :, :, c] - d[:, :, :, c - 1]).abs().mean().item() for c in cols]
    return max(jumps)


def test_blending_shrinks_the_seam_of_a_whole_image_pooling_model(device):
    """RCAN x2 pools over whatever it is given, so two tiles of a half dark, half bright image meet at a step; D = tiled - untiled."""
    m, s = _u8_models(device)['rcan']
    h, w, tile = 40, 56, (20, 28)
    x = ops.image_u8_to_nchw(_two_halves_image(1, h, w, seed=5).to(device), torch.float32)
    tiles = _plan(h, w, tile, 8)
    full = m(x).clone()
    jumps = {}
    for blend in (0, 4):
        d = tiling.upscale_tiled(m, x, s, tile=tile, halo=8, blend=blend).float() - full.float()
        jumps[blend] = _seam_jump(d.cpu(), tiles, s)
    print(f'MEASURE rcan x2 seam: largest mean |jump| of (tiled - untiled) across a seam line {jumps[0]:.3e} with blend 0, {jumps[4]:.3e} with blend 4')
    assert jumps[4] < jumps[0]
