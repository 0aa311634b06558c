"""Seam blending of the tiler (``upscale_tiled(blend=)``, DESIGN.md "Tile seams") on CPU tensors: the geometry function against the f64
restatement of the weights (tests/tile_blend_reference.py), the torch path of the accumulation with fake models and one real oracle, the
refusals, and the argument checks of ``rsa_tile_blend_accumulate`` (host only: nothing is launched)."""

import pytest
import torch

import tile_blend_reference as R
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.tiling import blend_window, plan_tiles, upscale_tiled
from resselt_amd.utils import synth

GRIDS = [(1, 1), (1, 3), (3, 1), (2, 2), (3, 4)]


def _up(s):
    return lambda t: t.repeat_interleave(s, -1).repeat_interleave(s, -2)


@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('grid', GRIDS)
def test_partition_of_unity_and_windows(grid, align):
    """The f64 weights of all tiles sum to 1 at every output pixel, and ``blend_window`` names exactly their supports and ramps."""
    rows, cols = grid
    h, w = rows * 20 + 1, cols * 22 + 3  # every tile at least 16 wide with align = 8: 2 * blend = 10 fits
    tiles = plan_tiles(h, w, rows, cols, halo=8, align=align)
    assert len(tiles) == rows * cols
    for scale in (1, 2, 3, 4):
        for blend in (1, 2, 5):
            total = torch.zeros(h * scale, w * scale, dtype=torch.float64)
            for t in tiles:
                wy, wx = R.axis_weights(t.y0, t.y1, h, blend, scale), R.axis_weights(t.x0, t.x1, w, blend, scale)
                total += wy[:, None] * wx[None, :]
                py0, py1, px0, px1, top, bottom, left, right = blend_window(t, h, w, blend, scale)
                for wgt, p0, p1, rise, fall in ((wy, py0, py1, top, bottom), (wx, px0, px1, left, right)):
                    assert torch.equal(torch.nonzero(wgt).flatten(), torch.arange(p0, p1)), (t, scale, blend)
                    inside = wgt[p0:p1]
                    assert bool((inside[:rise] < 1).all()) and bool((inside[p1 - p0 - fall :] < 1).all()) and bool((inside[rise : p1 - p0 - fall] == 1).all())
                    assert rise in (0, 2 * blend * scale) and fall in (0, 2 * blend * scale) and rise + fall <= p1 - p0
                assert (top == 0) == (t.y0 == 0) and (bottom == 0) == (t.y1 == h) and (left == 0) == (t.x0 == 0) and (right == 0) == (t.x1 == w)
            assert (total - 1).abs().max().item() <= 2.0**-50, (grid, align, scale, blend)


@pytest.mark.parametrize('grid,blend', [((2, 2), 1), ((2, 2), 4), ((3, 4), 5), ((1, 3), 2)])
def test_constant_image_stays_constant(grid, blend):
    rows, cols = grid
    h, w = rows * 20 + 1, cols * 22 + 3
    x = torch.full((2, 3, h, w), 0.7319, dtype=torch.float32)
    y = upscale_tiled(_up(3), x, 3, tile=(-(-h // rows), -(-w // cols)), halo=8, blend=blend)
    assert y.shape == (2, 3, 3 * h, 3 * w) and y.dtype == torch.float32
    assert ((y.double() - x[0, 0, 0, 0].double()).abs().max() / x[0, 0, 0, 0].double()).item() <= 2.0**-22


def _two_halves(n, h, w, seed):
    """A dark left half and a bright right half: tiles on either side have different means."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3, h, w), generator=g) * 0.1
    x[..., w // 2 :] += 0.8
    return x


def _jump(d):
    return max((d[..., 1:, :] - d[..., :-1, :]).abs().max().item(), (d[..., :, 1:] - d[..., :, :-1]).abs().max().item())


@pytest.mark.parametrize('blend', [1, 4])
def test_global_statistic_model_blends_the_tile_means(blend):
    """model = upsample(x) + mean(x), the mean over whatever the model is given (a tile with its halo).  blended - upsample(x) is then
    sum_t w_t * mean_t, and its largest step between neighbouring pixels is smaller than the step of the hard crop."""
    s, h, w = 2, 40, 56
    x = _two_halves(1, h, w, seed=5)
    means = []

    def model(t):
        m = t.double().mean().float()  # the f32 value the tile adds: recorded so the reference uses exactly it
        means.append(m.double())
        return _up(s)(t) + m

    tiles = plan_tiles(h, w, 2, 2, halo=8)
    y = upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend)
    assert len(means) == 4 and len({float(m) for m in means}) == 4
    want = sum(R.tile_weights(t, h, w, blend, s) * m for t, m in zip(tiles, means))
    d = y.double() - _up(s)(x).double()
    assert (d - want).abs().max().item() <= 2.0**-21 * max(1.0, y.abs().max().item())
    hard = upscale_tiled(model, x, s, tile=(20, 28), halo=8).double() - _up(s)(x).double()
    assert _jump(d) < _jump(hard), (_jump(d), _jump(hard))


def test_values_outside_the_bands_are_the_hard_crop_and_one_tile_is_untiled():
    s, h, w, blend = 2, 40, 56, 4
    x = _two_halves(2, h, w, seed=6)
    model = lambda t: _up(s)(t) + t.mean()  # noqa: E731
    tiles = plan_tiles(h, w, 2, 2, halo=8)
    band = R.band_mask(tiles, h, w, blend, s)
    assert 0 < int(band.sum()) < band.numel()
    soft, hard = upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend), upscale_tiled(model, x, s, tile=(20, 28), halo=8)
    assert torch.equal(soft[..., ~band], hard[..., ~band]) and not torch.equal(soft, hard)
    for dtype in (torch.float16, torch.bfloat16):  # the f32 sum is cast back to the model's dtype
        soft16 = upscale_tiled(model, x.to(dtype), s, tile=(20, 28), halo=8, blend=blend)
        assert soft16.dtype == dtype and torch.equal(soft16[..., ~band], upscale_tiled(model, x.to(dtype), s, tile=(20, 28), halo=8)[..., ~band])
    assert torch.equal(upscale_tiled(model, x, s, tile=(40, 56), halo=8, blend=blend), model(x))  # fits one tile: blend is ignored
    assert torch.equal(upscale_tiled(model, x, s, tile=(64, 64), halo=2, blend=50), model(x))


def test_u8_images_blend_in_f32_and_round_once():
    """uint8 [N, H, W, C] tiles: the codes enter as code / 255, the sum is rounded half to even; outside the bands nothing changes."""
    s, h, w, blend = 2, 40, 56, 4
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (2, h, w, 3), generator=g, dtype=torch.uint8)
    outs = []

    def model(t):  # upsample + a per-tile offset, in codes
        y = (_up(s)(t.permute(0, 3, 1, 2)).int() + int(t.float().mean()) // 8).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        outs.append(y)
        return y

    tiles = plan_tiles(h, w, 2, 2, halo=8)
    soft = upscale_tiled(model, img, s, tile=(20, 28), halo=8, blend=blend)
    want = R.compose(tiles, [R.image_as_f64(y) for y in outs], h, w, blend, s) * 255
    assert soft.dtype == torch.uint8 and soft.shape == (2, 2 * h, 2 * w, 3)
    got = soft.permute(0, 3, 1, 2).double()
    near_tie = ((want - want.floor()) - 0.5).abs() <= 1e-3
    assert torch.equal(got[~near_tie], want.round()[~near_tie]) and (got - want).abs().max().item() <= 0.5 + 1e-3
    band = R.band_mask(tiles, h, w, blend, s)
    assert torch.equal(soft.permute(0, 3, 1, 2)[..., ~band], upscale_tiled(model, img, s, tile=(20, 28), halo=8).permute(0, 3, 1, 2)[..., ~band])


def test_refusals_name_the_offending_value():
    x = torch.rand(1, 3, 40, 56)
    with pytest.raises(ValueError, match='-1'):
        upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=8, blend=-1)
    with pytest.raises(ValueError, match='-3'):
        tiling.upscale(None, torch.zeros(4, 4, 3, dtype=torch.uint8), blend=-3)  # before anything touches the image
    with pytest.raises(ValueError, match=r'blend = 9 exceeds the halo of 8'):
        upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=8, blend=9)
    # the effective halo: 5 rounded up to align = 8
    assert upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=5, align=8, blend=8).shape == (1, 3, 80, 112)
    with pytest.raises(ValueError, match=r'blend = 9 exceeds the halo of 8'):
        upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=5, align=8, blend=9)
    with pytest.raises(ValueError, match=r'2 \* blend = 22 exceeds the tile extent of 20'):
        upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=32, blend=11)
    with pytest.raises(ValueError, match=r'2 \* blend = 30 exceeds the tile extent of 28'):
        upscale_tiled(_up(2), x, 2, tile=(40, 28), halo=32, blend=15)  # one row of tiles: only the columns count
    assert upscale_tiled(_up(2), x[:, :, :10], 2, tile=(10, 19), halo=8, blend=8).shape == (1, 3, 20, 112)  # 2 * blend > 10 rows, but one row of tiles
    assert not hasattr(tiling.TileParallel(_up(2), 2), 'blend')


def test_oracle_run_matches_the_f64_composition_of_its_own_tiles():
    from oracle.compact import compact_forward

    sd = synth.compact_state_dict(num_feat=16, num_conv=3, upscale=4, seed=12)
    outs = []

    def model(t):
        with torch.no_grad():
            y = compact_forward(sd, t)
        outs.append(y)
        return y

    s, h, w, blend = 4, 40, 56, 4
    x = synth.synth_input((1, 3, h, w), seed=12)
    tiles = plan_tiles(h, w, 2, 2, halo=8)
    y = upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend)
    assert len(outs) == 4 and y.shape == (1, 3, s * h, s * w) and y.dtype == outs[0].dtype
    want = R.compose(tiles, outs, h, w, blend, s)
    err = (y.double() - want).abs().max().item()
    print(f'MEASURE oracle run: max-abs against the f64 composition {err:.3e} (|y|max {want.abs().max():.3f})')
    assert err <= 2.0**-21 * max(1.0, want.abs().max().item())
    # the halo of 8 does not cover this network's reach: the tiles do differ inside the bands, so the blend is not a no-op
    assert (y - upscale_tiled(model, x, s, tile=(20, 28), halo=8)).abs().max().item() > 1e-6


E_ARG, E_ALIGN = -1, -3
SRC, ACC = 0x100000, 0x900000  # fake 16-byte aligned addresses: every call below is refused before a launch


def _args(**over):
    a = dict(src=SRC, src_dtype=L.F32, batch=1, C=3, win_h=16, win_w=24, src_h=40, src_w=48, src_y=8, src_x=8, acc=ACC, acc_h=64, acc_w=96,
             acc_y=4, acc_x=12, ramp_top=8, ramp_bottom=0, ramp_left=8, ramp_right=8, stream=None)  # fmt: skip
    assert list(a) == [k for k, _ in L.INTERNAL['rsa_tile_blend_accumulate'][1]]
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize('over,status', [
    (dict(src=None), E_ARG), (dict(acc=None), E_ARG), (dict(src_dtype=4), E_ARG), (dict(src_dtype=-1), E_ARG),
    (dict(batch=0), E_ARG), (dict(C=0), E_ARG), (dict(win_h=0), E_ARG), (dict(win_w=-2), E_ARG), (dict(src_h=0), E_ARG), (dict(acc_w=0), E_ARG),
    (dict(src_y=-1), E_ARG), (dict(src_y=25), E_ARG), (dict(src_x=25), E_ARG), (dict(win_w=41), E_ARG),  # the window leaves the source
    (dict(acc_y=-1), E_ARG), (dict(acc_y=49), E_ARG), (dict(acc_x=73), E_ARG), (dict(acc_x=2**31 - 8), E_ARG),  # ... the accumulator
    (dict(ramp_top=-1), E_ARG), (dict(ramp_top=17), E_ARG), (dict(ramp_bottom=17), E_ARG), (dict(ramp_left=25), E_ARG), (dict(ramp_right=25), E_ARG),
    (dict(batch=70000, C=1), E_ARG),
    (dict(acc=ACC + 4), E_ALIGN), (dict(src=SRC + 2), E_ALIGN), (dict(src=SRC + 1, src_dtype=L.F16), E_ALIGN),
])  # fmt: skip
def test_argument_checks_return_before_any_launch(over, status):
    lib = L.load()
    assert lib.rsa_tile_blend_accumulate(*_args(**over)) == status, over
    assert b'rsa_tile_blend_accumulate' in lib.rsa_last_error_string()
