"""``upscale(out_size= / out_scale=)`` on CPU tensors: ``resample_table`` against torch's f64 antialiased interpolation, the
torch path of ``upscale`` / ``upscale_tiled`` with fake models and one real oracle against the f64 interpolation of the native frame, the
refusals, and the argument checks of ``rsa_resample`` (host only: nothing is launched).

Expected values come from ``F.interpolate(..., antialias=True)`` in float64 (tests/resample_reference.py), never from the code under
test.  Float results are within ``B = (T_h + T_w + 4) * 2^-24 * S_h * S_w * max(1, |x|max)`` (computed per case from the tables), 8-bit
results within ``0.5 + 255 * B`` of ``255 * clamp(v64)``; where the native frame is the f32 sum of a blend, ``2^-21 * S_h * S_w * max(1,
|x|max)`` is added for that sum's own rounding (tests/test_tile_blend_kernels_gpu.py derives the 2^-21)."""

import pytest
import torch

import resample_reference as R
import tile_blend_reference as TB
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.tiling import plan_tiles, resample_table, upscale_tiled
from resselt_amd.utils import synth

FILTERS = ['bicubic', 'bilinear']
# (h, w) -> (rows, columns): non-integer shrinks, the ratio limit, enlargement, identity, a 1 x 1 output, one axis kept
SIZE_PAIRS = [((24, 40), (9, 13)), ((37, 29), (5, 4)), ((64, 64), (8, 8)), ((16, 20), (24, 50)), ((8, 8), (8, 8)), ((8, 5), (1, 1)),
              ((12, 20), (12, 7)), ((9, 14), (23, 14))]  # fmt: skip


def _up(s):
    return lambda t: t.repeat_interleave(s, -1).repeat_interleave(s, -2)


class _U8Model:
    """A fake of a ``supports_u8`` model: uint8 [N, H, W, C] in, the image repeated ``s`` times out, plus the tile's mean // 8 codes."""

    supports_u8 = True

    def __init__(self, s):
        self.s, self.outs = s, []

    def __call__(self, t):
        y = t.repeat_interleave(self.s, 1).repeat_interleave(self.s, 2)
        y = (y.int() + int(t.float().mean()) // 8).clamp(0, 255).to(torch.uint8)
        self.outs.append(y)
        return y


@pytest.mark.parametrize('filter', FILTERS)
@pytest.mark.parametrize('src,dst', SIZE_PAIRS)
def test_tables_restate_torch_in_f64(src, dst, filter):
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    x = torch.rand((2, 3, *src), generator=g, dtype=torch.float64) * 4 - 2
    ty, tx = resample_table(src[0], dst[0], filter), resample_table(src[1], dst[1], filter)
    for (start, weight), n_in, n_out in ((ty, src[0], dst[0]), (tx, src[1], dst[1])):
        assert start.dtype == torch.int32 and weight.dtype == torch.float32 and start.shape == (n_out,) and weight.shape[0] == n_out
        taps = weight.shape[1]
        assert 1 <= taps <= min(n_in, 33 if filter == 'bicubic' else 17)
        assert int(start.min()) >= 0 and int((start + taps).max()) <= n_in
        assert (weight.double().sum(1) - 1).abs().max().item() <= 2.0**-22
        if n_in == n_out:  # identity: exactly one-hot
            assert bool(((weight == 1).sum(1) == 1).all()) and bool(((weight == 0).sum(1) == taps - 1).all())
            assert torch.equal(start + weight.argmax(1).int(), torch.arange(n_out, dtype=torch.int32))
    # the f32 rounding of the weights is no part of the restatement: compare with weights rebuilt in f64 from the same rows
    want = R.interpolate64(x, dst, filter)
    got = R.apply_tables(x, ty, tx)
    err32 = (got - want).abs().max().item()
    assert err32 <= R.bound(ty, tx, x.abs().max().item())
    ty64, tx64 = _table64(src[0], dst[0], filter), _table64(src[1], dst[1], filter)
    assert torch.equal(ty64[0], ty[0]) and torch.equal(ty64[1].float(), ty[1]) and torch.equal(tx64[0], tx[0]) and torch.equal(tx64[1].float(), tx[1])
    err = (R.apply_tables(x, ty64, tx64) - want).abs().max().item()
    print(f'MEASURE table {filter} {src}->{dst}: f64 weights {err:.2e}, f32 weights {err32:.2e} against torch f64')
    assert err <= 1e-12


def _table64(n_in, n_out, filter):
    """The table before its one rounding to f32: these f64 weights are what the test pins to torch."""
    start, weight = resample_table(n_in, n_out, filter, dtype=torch.float64)
    assert weight.dtype == torch.float64
    return start, weight


@pytest.mark.parametrize('filter', FILTERS)
@pytest.mark.parametrize('kw,size', [(dict(out_scale=2), (80, 112)), (dict(out_scale=3), (120, 168)), (dict(out_scale=2.5), (100, 140)),
                                     (dict(out_size=(40, 56)), (40, 56)), (dict(out_size=(33, 300)), (33, 300)), (dict(out_scale=0.5), (20, 28))])  # fmt: skip
def test_upscale_tiled_float_against_torch_f64_of_the_native_frame(kw, size, filter):
    s, h, w = 4, 40, 56
    x = synth.synth_input((2, 3, h, w), seed=21)
    model = _up(s)
    native = upscale_tiled(model, x, s, tile=(20, 28), halo=8)
    want = R.interpolate64(native, size, filter)
    ty, tx = resample_table(s * h, size[0], filter), resample_table(s * w, size[1], filter)
    b = R.bound(ty, tx, native.abs().max().item())
    for tile in ((20, 28), (64, 64)):  # hard-crop tiles, and an image that fits one tile
        y = upscale_tiled(model, x, s, tile=tile, halo=8, resample=filter, **kw)
        assert y.dtype == torch.float32 and tuple(y.shape) == (2, 3, *size)
        err = (y.double() - want).abs().max().item()
        print(f'MEASURE fake x4 {kw} {filter} tile {tile}: worst error {err / b:.3f} of the bound {b:.2e}')
        assert err <= b
    y16 = upscale_tiled(model, x.half(), s, tile=(20, 28), halo=8, resample=filter, **kw)  # the model's dtype comes back: one more rounding
    want16 = R.interpolate64(upscale_tiled(model, x.half(), s, tile=(20, 28), halo=8), size, filter)
    assert y16.dtype == torch.float16 and (y16.double() - want16).abs().max().item() <= b + 2.0**-11 * max(1.0, want16.abs().max().item())


@pytest.mark.parametrize('filter', FILTERS)
def test_upscale_tiled_blend_resamples_the_f32_sum(filter):
    s, h, w, blend, size = 2, 40, 56, 4, (60, 100)
    x = synth.synth_input((1, 3, h, w), seed=22)
    outs = []

    def model(t):
        y = _up(s)(t) + t.mean()
        outs.append(y)
        return y

    tiles = plan_tiles(h, w, 2, 2, halo=8)
    y = upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend, out_size=size, resample=filter)
    native = TB.compose(tiles, outs[:4], h, w, blend, s)
    want = R.interpolate64(native, size, filter)
    ty, tx = resample_table(s * h, size[0], filter), resample_table(s * w, size[1], filter)
    xmax = native.abs().max().item()
    b = R.bound(ty, tx, xmax) + 2.0**-21 * R.abs_row_sum(ty) * R.abs_row_sum(tx) * max(1.0, xmax)
    err = (y.double() - want).abs().max().item()
    print(f'MEASURE fake x2 blend {filter}: worst error {err / b:.3f} of the bound {b:.2e}')
    assert y.dtype == torch.float32 and tuple(y.shape) == (1, 3, *size) and err <= b


@pytest.mark.parametrize('tile,blend', [(None, 0), ((20, 28), 0), ((20, 28), 4)])
@pytest.mark.parametrize('kw,size', [(dict(out_scale=1.5), (60, 84)), (dict(out_size=(40, 56)), (40, 56)), (dict(out_size=(100, 31)), (100, 31))])
def test_upscale_of_an_8_bit_model_rounds_once_after_the_filter(kw, size, tile, blend):
    s, h, w = 2, 40, 56
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (2, h, w, 3), generator=g, dtype=torch.uint8)
    m = _U8Model(s)
    got = tiling.upscale(m, img, tile=tile, halo=8, scale=s, blend=blend, **kw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, *size, 3)
    if blend:
        tiles = plan_tiles(h, w, 2, 2, halo=8)
        native, extra = TB.compose(tiles, [R.image_as_f64(y) for y in m.outs[:4]], h, w, blend, s), 2.0**-21
    else:
        native, extra = R.image_as_f64(tiling.upscale(_U8Model(s), img, tile=tile, halo=8, scale=s)), 0.0
    want = R.interpolate64(native, size, 'bicubic')
    ty, tx = resample_table(s * h, size[0], 'bicubic'), resample_table(s * w, size[1], 'bicubic')
    b = R.bound(ty, tx, 1.0) + extra * R.abs_row_sum(ty) * R.abs_row_sum(tx)
    err = R.image_error(got, want)
    print(f'MEASURE fake 8-bit x2 {kw} tile {tile} blend {blend}: {err:.4f} codes (allowed {0.5 + 255 * b:.4f})')
    assert err <= 0.5 + 255 * b
    one = tiling.upscale(_U8Model(s), img[0], tile=tile, halo=8, scale=s, blend=blend, **kw)  # [H, W, C] in, [rows, columns, C] out
    assert one.dim() == 3 and torch.equal(one, tiling.upscale(_U8Model(s), img[:1], tile=tile, halo=8, scale=s, blend=blend, **kw)[0])


def test_native_size_and_no_argument_change_nothing():
    s, h, w = 4, 40, 56
    x = synth.synth_input((1, 3, h, w), seed=23)
    model = lambda t: _up(s)(t) + t.mean()  # noqa: E731
    for blend in (0, 4):
        old = upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend)
        assert torch.equal(upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend, out_size=(s * h, s * w)), old)
        assert torch.equal(upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend, out_scale=s, resample='bilinear'), old)
        img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8)
        old8 = tiling.upscale(_U8Model(s), img, tile=(20, 28), halo=8, scale=s, blend=blend)
        assert torch.equal(tiling.upscale(_U8Model(s), img, tile=(20, 28), halo=8, scale=s, blend=blend, out_size=(s * h, s * w)), old8)
        assert torch.equal(tiling.upscale(_U8Model(s), img, tile=(20, 28), halo=8, scale=s, blend=blend, out_scale=float(s)), old8)
        assert torch.equal(tiling.upscale(_U8Model(s), img, scale=s, out_scale=s), tiling.upscale(_U8Model(s), img, scale=s))


def test_refusals():
    x = torch.rand(1, 3, 40, 56)
    img = torch.zeros(40, 56, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='not both'):
        upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=8, out_size=(10, 10), out_scale=2)
    with pytest.raises(ValueError, match='not both'):
        tiling.upscale(None, img, out_size=(10, 10), out_scale=2)  # before anything touches the image or the model
    for bad in (0, -1.5):
        with pytest.raises(ValueError, match='out_scale'):
            upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=8, out_scale=bad)
        with pytest.raises(ValueError, match='out_scale'):
            tiling.upscale(None, img, out_scale=bad)
    for bad in ((0, 10), (10, -3), (10,), (2.5, 10)):
        with pytest.raises(ValueError, match='out_size'):
            upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=8, out_size=bad)
        with pytest.raises(ValueError, match='out_size'):
            tiling.upscale(None, img, out_size=bad)
    with pytest.raises(ValueError, match='lanczos'):
        upscale_tiled(_up(2), x, 2, tile=(20, 28), halo=8, out_scale=1, resample='lanczos')
    with pytest.raises(ValueError, match='lanczos'):
        tiling.upscale(None, img, resample='lanczos')  # refused even where nothing would be resampled
    with pytest.raises(ValueError, match='lanczos'):
        resample_table(16, 8, 'lanczos')
    # 80 rows -> 9 is a ratio of 8.9; 80 -> 10 is the limit and runs.  The model must not have run when the ratio is refused.
    ran = []

    def model(t):
        ran.append(1)
        return _up(2)(t)

    with pytest.raises(ValueError, match='more than 8'):
        upscale_tiled(model, x, 2, tile=(20, 28), halo=8, out_size=(9, 112))
    with pytest.raises(ValueError, match='more than 8'):
        tiling.upscale(_U8Model(2), img, scale=2, out_size=(80, 13))
    assert not ran
    assert upscale_tiled(model, x, 2, tile=(20, 28), halo=8, out_size=(10, 14)).shape == (1, 3, 10, 14)
    with pytest.raises(ValueError, match='more than 8'):
        resample_table(65, 8, 'bilinear')
    with pytest.raises(ValueError):
        resample_table(8, 0, 'bicubic')
    assert resample_table(3, 4000, 'bicubic')[1].shape == (4000, 3)  # any enlargement
    assert not hasattr(tiling.TileParallel(_up(2), 2), 'out_size')


def test_oracle_run_matches_torch_f64_of_its_own_native_frame():
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
    for kw, size in ((dict(out_scale=2), (80, 112)), (dict(out_size=(121, 77)), (121, 77))):
        ty, tx = resample_table(s * h, size[0], 'bicubic'), resample_table(s * w, size[1], 'bicubic')
        # hard crop: the native frame is what the same call returns without out_size
        native = upscale_tiled(model, x, s, tile=(20, 28), halo=8)
        y = upscale_tiled(model, x, s, tile=(20, 28), halo=8, **kw)
        b = R.bound(ty, tx, native.abs().max().item())
        err = (y.double() - R.interpolate64(native, size, 'bicubic')).abs().max().item()
        print(f'MEASURE oracle compact x4 {kw} hard crop: worst error {err / b:.3f} of the bound {b:.2e}')
        assert y.dtype == native.dtype and tuple(y.shape) == (1, 3, *size) and err <= b
        # blend: the native frame is the f64 composition of the tiles the model produced in this very call
        del outs[:]
        y = upscale_tiled(model, x, s, tile=(20, 28), halo=8, blend=blend, **kw)
        native = TB.compose(tiles, outs, h, w, blend, s)
        xmax = native.abs().max().item()
        b = R.bound(ty, tx, xmax) + 2.0**-21 * R.abs_row_sum(ty) * R.abs_row_sum(tx) * max(1.0, xmax)
        err = (y.double() - R.interpolate64(native, size, 'bicubic')).abs().max().item()
        print(f'MEASURE oracle compact x4 {kw} blend {blend}: worst error {err / b:.3f} of the bound {b:.2e}')
        assert len(outs) == 4 and err <= b


E_ARG, E_ALIGN = -1, -3
SRC, DST, SY, WY, SX, WX = 0x100000, 0x900000, 0x200000, 0x300000, 0x400000, 0x500000  # fake aligned addresses: every call is refused before a launch


def _args(**over):
    a = dict(src=SRC, src_dtype=L.F32, batch=1, C=3, src_h=40, src_w=48, dst=DST, dst_dtype=L.U8, dst_h=20, dst_w=30, start_y=SY, weight_y=WY,
             taps_y=9, start_x=SX, weight_x=WX, taps_x=8, stream=None)  # fmt: skip
    assert list(a) == [k for k, _ in L.INTERNAL['rsa_resample'][1]]
    a.update(over)
    return list(a.values())


def test_internal_row_names_the_arguments_in_the_order_of_the_entry_point():
    import ctypes as C

    restype, params = L.INTERNAL['rsa_resample']
    assert restype is C.c_int
    assert [k for k, _ in params] == ['src', 'src_dtype', 'batch', 'C', 'src_h', 'src_w', 'dst', 'dst_dtype', 'dst_h', 'dst_w', 'start_y', 'weight_y',
                                      'taps_y', 'start_x', 'weight_x', 'taps_x', 'stream']  # fmt: skip
    assert [t for k, t in params if k.startswith(('src_', 'dst_', 'taps')) or k in ('batch', 'C')] == [C.c_int32] * 10
    assert [t for k, t in params if k in ('src', 'dst', 'start_y', 'weight_y', 'start_x', 'weight_x', 'stream')] == [C.c_void_p] * 7
    assert 'rsa_resample' not in L.SIGNATURES and 'rsa_resample' not in L.EXTENSIONS  # no header declares it


@pytest.mark.parametrize('over,status', [
    (dict(src=None), E_ARG), (dict(dst=None), E_ARG), (dict(start_y=None), E_ARG), (dict(weight_y=None), E_ARG), (dict(start_x=None), E_ARG),
    (dict(weight_x=None), E_ARG), (dict(src_dtype=4), E_ARG), (dict(src_dtype=-1), E_ARG), (dict(dst_dtype=4), E_ARG), (dict(dst_dtype=-1), E_ARG),
    (dict(batch=0), E_ARG), (dict(C=0), E_ARG), (dict(src_h=0), E_ARG), (dict(src_w=-2), E_ARG), (dict(dst_h=0), E_ARG), (dict(dst_w=0), E_ARG),
    (dict(taps_y=0), E_ARG), (dict(taps_x=-1), E_ARG), (dict(taps_y=34), E_ARG), (dict(taps_x=34), E_ARG),
    (dict(batch=70000, C=1), E_ARG), (dict(batch=300, C=300), E_ARG), (dict(dst_h=16 * 65535 + 1, src_h=2**24), E_ARG),  # the grid
    (dict(src_h=4000, dst_h=20, taps_y=33), E_ARG),  # a band of 15 * 200 rows: no LDS holds it
    (dict(src=SRC + 2), E_ALIGN), (dict(src=SRC + 1, src_dtype=L.F16), E_ALIGN), (dict(dst=DST + 1, dst_dtype=L.BF16), E_ALIGN),
    (dict(dst=DST + 2, dst_dtype=L.F32), E_ALIGN), (dict(start_y=SY + 2), E_ALIGN), (dict(weight_x=WX + 1), E_ALIGN),
])  # fmt: skip
def test_argument_checks_return_before_any_launch(over, status):
    lib = L.load()
    assert lib.rsa_resample(*_args(**over)) == status, over
    assert b'rsa_resample' in lib.rsa_last_error_string()
