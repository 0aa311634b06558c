"""The still-image formats of ``upscale_rgba`` on CPU tensors: the f32 torch path of ``ops.image_to_nchw_alpha`` /
``ops.nchw_to_image_alpha`` against the f64 definition (tests/rgba_reference.py), hand-checkable pins, ``upscale_rgba`` with fake models, the
refusals, and the argument checks of the two entry points (host only: nothing is launched).

Bounds (rgba_reference.py derives them): a value read is within ``2^-24 + 8 bleed 2^-24`` (plus one rounding of an f16 / bf16 destination) of
the f64 value, a written code within ``0.5 + M * 4 * 2^-24`` of the unrounded f64 target.  Where the frame that is written comes out of an f32
blend sum or an f32 resampling, that step's own bound (tests/test_tile_blend.py, tests/test_resample.py) is added, times ``M``."""

import ctypes as C

import pytest
import torch

import resample_reference as R
import resselt_amd
import rgba_reference as G
import tile_blend_reference as TB
from resselt_amd import tiling
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.tiling import plan_tiles, resample_table

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.mark.parametrize('bits', [8, 16])
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_torch_path_reads_as_the_definition(c, bits):
    for n, h, w, bleed in ((2, 13, 17, 16), (1, 7, 9, 3), (1, 1, 1, 8), (2, 5, 4, 0)):
        img = G.random_image(n, h, w, c, bits, seed=h * w + c, transparent=0.8)
        for cm in ((1, 3) if c <= 2 else (3,)):
            for mode in ('model', 'resample'):
                for dtype in DTYPES:
                    x, a, flags = ops.image_to_nchw_alpha(img, cm, mode, bleed, dtype)
                    what = f'torch read C={c} {bits} bits Cm={cm} {mode} bleed {bleed} {n}x{h}x{w}'
                    assert x.dtype == dtype and x.is_contiguous()
                    col, a64, f64 = G.read64(img, bleed)
                    if G.has_alpha(c):
                        assert flags.dtype == torch.int32 and torch.equal(flags.bool(), f64), what
                    else:
                        assert flags is None and a is None
                    G.assert_read(x, img, cm, mode, bleed, what)
                    if G.has_alpha(c) and mode == 'resample':
                        assert a.dtype == torch.float32 and tuple(a.shape) == (n, 1, h, w) and (a.double() - a64).abs().max().item() <= G.U, what
    one = ops.image_to_nchw_alpha(img[0], 3, 'model', 4, torch.float32)[0]  # [H, W, C]: a batch of one
    assert torch.equal(one, ops.image_to_nchw_alpha(img[:1], 3, 'model', 4, torch.float32)[0])


def test_f32_and_f64_agree_on_the_known_sets():
    """The pixels the torch path changed are exactly the ones the f64 definition fills, pass by pass."""
    img = G.random_image(1, 40, 50, 4, 8, seed=3, transparent=0.97)
    stored = G.codes_of(img)[:, :3].double() / 255
    for passes in (1, 2, 5, 16):
        x, _, _ = ops.image_to_nchw_alpha(img, 3, 'resample', passes, torch.float32)
        _, known = G.bleed64(stored, G.codes_of(img)[:, 3:] > 0, passes)
        filled = known & ~(G.codes_of(img)[:, 3:] > 0)
        changed = (x - G.codes_of(img)[:, :3].float() / 255).abs().amax(1, keepdim=True) > 0  # against the f32 quotient a copy gives
        assert not bool((changed & ~filled).any()), passes  # (a filled pixel may by chance equal its stored colour)
        assert bool(filled.any()) and bool(changed.any())


@pytest.mark.parametrize('bits', [8, 16])
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_torch_path_writes_as_the_definition(c, bits):
    for n, h, w in ((2, 6, 10), (1, 1, 1), (1, 3, 5)):
        for cm in ((1, 3) if c <= 2 else (3,)):
            color = G.random_source(n, cm, h, w, seed=h + w + c)
            for ca in (None, 1, cm):
                alpha = None if ca is None else G.random_source(n, ca, h, w, seed=7 + ca)
                for dtype in DTYPES:
                    got = ops.nchw_to_image_alpha(color.to(dtype), None if alpha is None else alpha.to(dtype), c, bits)
                    assert tuple(got.shape) == (n, h, w, c) and got.dtype == G.DEPTHS[bits][0]
                    G.assert_written(got, color, alpha, f'torch write C={c} {bits} bits Cm={cm} Ca={ca} {dtype} {n}x{h}x{w}')
                    if G.has_alpha(c) and ca is None:
                        assert set(got[..., c - 1].to(torch.int32).flatten().tolist()) == {G.DEPTHS[bits][1]}


def test_one_known_pixel_in_each_corner_colours_a_17_by_17_square():
    h, w, bleed = 48, 56, 16
    img = G.random_image(1, h, w, 4, 8, seed=1).to(torch.int32)
    img[..., 3] = 0
    corners = {(0, 0): (10, 200, 30), (0, w - 1): (255, 0, 7), (h - 1, 0): (1, 2, 3), (h - 1, w - 1): (90, 91, 92)}
    for (y, x), rgb in corners.items():
        img[0, y, x] = torch.tensor([*rgb, 1 + y % 3], dtype=torch.int32)
    img = img.to(torch.uint8)
    got, _, flags = ops.image_to_nchw_alpha(img, 3, 'resample', bleed, torch.float32)
    want = img[..., :3].permute(0, 3, 1, 2).float() / 255  # the stored colour ...
    inside = torch.zeros(h, w, dtype=torch.bool)
    for (y, x), rgb in corners.items():  # ... but for a 17 x 17 square of its corner's own colour around every known pixel
        ys, xs = slice(max(y - bleed, 0), y + bleed + 1), slice(max(x - bleed, 0), x + bleed + 1)
        want[0, :, ys, xs] = (torch.tensor(rgb).float() / 255).reshape(3, 1, 1)
        assert (ys.stop - ys.start if y == 0 else y + 1 - ys.start) == 17
        inside[ys, xs] = True
    assert int(inside.sum()) == 4 * 17 * 17 and flags.tolist() == [1]
    assert torch.equal(got[0][:, ~inside], want[0][:, ~inside])  # nothing else moved
    assert (got - want).abs().max().item() <= G.U + G.b_bleed(bleed)  # a mean of equal colours is that colour, up to the roundings of the mean
    ref, _, _ = G.read64(img, bleed)
    assert (ref - want.double()).abs().max().item() <= 2.0**-24  # (want is an f32 quotient)


def test_transparent_opaque_alpha_and_depth_pins():
    img = G.random_image(2, 9, 12, 4, 8, seed=5)
    stored = img[..., :3].permute(0, 3, 1, 2).float() / 255
    for value, flag in ((0, 1), (255, 0)):  # a fully transparent image and a fully opaque one come back unchanged
        im = G.with_alpha(img, value)
        x, a, flags = ops.image_to_nchw_alpha(im, 3, 'resample', 16, torch.float32)
        assert torch.equal(x, stored) and flags.tolist() == [flag, flag] and torch.equal(a, torch.full_like(a, value / 255))
    for bleed in (0, 1, 16):  # alpha is never modified, nor colour under alpha > 0; bleed = 0 copies
        x, a, _ = ops.image_to_nchw_alpha(img, 3, 'resample', bleed, torch.float32)
        assert torch.equal(a[:, 0], img[..., 3].float() / 255)
        visible = (img[..., 3] > 0)[:, None].expand_as(x)
        assert torch.equal(x[visible], stored[visible])
        if bleed == 0:
            assert torch.equal(x, stored)
        back = ops.nchw_to_image_alpha(x, a, 4, 8)
        assert torch.equal(back[..., 3], img[..., 3]) and torch.equal(back[visible[:, 0]], img[visible[:, 0]])
    full = torch.full((1, 2, 3, 4), 255, dtype=torch.uint8)  # 8-bit -> 16-bit of code 255 is 65535
    x, a, _ = ops.image_to_nchw_alpha(full, 3, 'resample', 8, torch.float32)
    assert set(ops.nchw_to_image_alpha(x, a, 4, 16).to(torch.int32).flatten().tolist()) == {65535}
    half = torch.full((1, 2, 3, 1), 128, dtype=torch.uint8)  # 128 / 255 * 65535 = 32896 exactly
    assert set(ops.nchw_to_image_alpha(ops.image_to_nchw_alpha(half, 1, 'model', 0, torch.float32)[0], None, 1, 16).to(torch.int32).flatten().tolist()) == {32896}


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


@pytest.mark.parametrize('tile,blend', [(None, 0), (TILE, 0), (TILE, 4)])
@pytest.mark.parametrize('c,bits,out_bits,dtype', [(4, 8, None, torch.float32), (4, 8, 16, torch.float32), (2, 16, None, torch.float16), (4, 16, 8, torch.bfloat16),
                                                   (3, 8, None, torch.float32), (1, 16, None, torch.float32)])  # fmt: skip
def test_upscale_rgba_with_a_cpu_callable(tile, blend, c, bits, out_bits, dtype):
    n, h, w, s, bleed = 2, 24, 40, 2, 5
    img = G.random_image(n, h, w, c, bits, seed=11)
    for mode in ('model', 'resample'):
        m = _Fake(s)
        got = resselt_amd.upscale_rgba(m, img, alpha=mode, bleed=bleed, out_bits=out_bits, tile=tile, halo=HALO, blend=blend, dtype=dtype, scale=s)
        what = f'fake x{s} C={c} {bits}->{out_bits or bits} {dtype} {mode} tile {tile} blend {blend}'
        assert tuple(got.shape) == (n, h * s, w * s, c) and got.dtype == G.DEPTHS[out_bits or bits][0]
        batch = 2 * n if (G.has_alpha(c) and mode == 'model') else n  # 'model': alpha rides as N further batch entries of the same call
        assert all(t.shape[0] == batch and t.dtype == dtype for t in m.ins), what
        if tile is None:
            G.assert_read(m.ins[0], img, 3, mode, bleed, what)
        native, extra = _native(m, h, w, s, tile, blend)
        if not G.has_alpha(c):
            G.assert_written(got, native, None, what, extra=extra)
        elif mode == 'model':
            G.assert_written(got, native[:n], native[n:], what, extra=extra)
        else:
            a64 = G.read64(img, bleed)[1]
            ty, tx = resample_table(h, s * h, 'bicubic'), resample_table(w, s * w, 'bicubic')
            G.assert_written(got[..., : c - 1].contiguous(), native, None, what + ' colour', extra=extra)
            alpha_img = got[..., c - 1 :].contiguous()
            target = R.interpolate64(a64, (s * h, s * w), 'bicubic').clamp(0, 1) * G.DEPTHS[out_bits or bits][1]
            err = G.code_error(alpha_img, target.permute(0, 2, 3, 1))
            assert err <= G.write_bound(out_bits or bits, R.bound(ty, tx, 1.0) + G.U), (what, err)
    m1 = _Fake(s)  # [H, W, C] in, [H, W, C] out
    one = resselt_amd.upscale_rgba(m1, img[0], tile=tile, halo=HALO, blend=blend, dtype=dtype, scale=s)
    assert one.dim() == 3 and tuple(one.shape) == (h * s, w * s, c)


def test_the_opaque_shortcut_calls_the_model_with_n_and_delivers_all_max_alpha():
    n, h, w, s = 2, 10, 14, 2
    for c, bits in ((4, 8), (2, 16)):
        img = G.with_alpha(G.random_image(n, h, w, c, bits, seed=2), G.DEPTHS[bits][1])
        rgb = img[..., : c - 1].contiguous()
        for mode in ('model', 'resample'):
            m, plain = _Fake(s), _Fake(s)
            got = resselt_amd.upscale_rgba(m, img, alpha=mode, dtype=torch.float32, scale=s, out_bits=16)
            assert [t.shape[0] for t in m.ins] == [n]
            assert set(got[..., c - 1].to(torch.int32).flatten().tolist()) == {65535}
            want = resselt_amd.upscale_rgba(plain, rgb, dtype=torch.float32, scale=s, out_bits=16)  # what the image without alpha costs and gives
            assert torch.equal(got[..., : c - 1].to(torch.int32), want.to(torch.int32)) and torch.equal(m.ins[0], plain.ins[0])
        semi = G.with_alpha(img, G.DEPTHS[bits][1] - 1)  # one code below the maximum everywhere: no shortcut
        m = _Fake(s)
        resselt_amd.upscale_rgba(m, semi, alpha='model', dtype=torch.float32, scale=s)
        assert [t.shape[0] for t in m.ins] == [2 * n]


@pytest.mark.parametrize('tile,blend', [(None, 0), (TILE, 4)])
@pytest.mark.parametrize('okw,size', [(dict(out_size=(30, 52)), (30, 52)), (dict(out_scale=1.5), (36, 60)), (dict(out_size=(100, 90), resample='bilinear'), (100, 90))])
def test_upscale_rgba_out_size_resamples_before_the_one_rounding(tile, blend, okw, size):
    n, h, w, s = 1, 24, 40, 2
    img = G.random_image(n, h, w, 4, 8, seed=12)
    m = _Fake(s)
    got = tiling.upscale_rgba(m, img, out_bits=16, tile=tile, halo=HALO, blend=blend, dtype=torch.float32, scale=s, **okw)
    assert tuple(got.shape) == (n, *size, 4)
    native, extra = _native(m, h, w, s, tile, blend)
    filter = okw.get('resample', 'bicubic')
    ty, tx = resample_table(s * h, size[0], filter), resample_table(s * w, size[1], filter)
    extra = extra * R.abs_row_sum(ty) * R.abs_row_sum(tx) + R.bound(ty, tx, native.abs().max().item())
    frame = R.interpolate64(native, size, filter)
    G.assert_written(got, frame[:n], frame[n:], f'fake x2 rgba8->16 {okw} tile {tile} blend {blend}', extra=extra)
    same = tiling.upscale_rgba(_Fake(s), img, out_bits=16, tile=tile, halo=HALO, blend=blend, dtype=torch.float32, scale=s, out_size=(s * h, s * w))
    plain = tiling.upscale_rgba(_Fake(s), img, out_bits=16, tile=tile, halo=HALO, blend=blend, dtype=torch.float32, scale=s)
    assert torch.equal(same.to(torch.int32), plain.to(torch.int32))  # the native size changes nothing


class _Info:
    def __init__(self, cin, cout, upscale=2):
        self.in_channels, self.out_channels, self.upscale = cin, cout, upscale


class _WithInfo(_Fake):
    def __init__(self, cin, cout):
        super().__init__(2)
        self.parameters_info = _Info(cin, cout)


def test_model_channels():
    gray = G.random_image(1, 8, 10, 2, 8, seed=4)
    for cm in (1, 3):  # a gray image on a one- and on a three-channel model
        m = _WithInfo(cm, cm)
        got = tiling.upscale_rgba(m, gray, dtype=torch.float32, bleed=2)
        assert tuple(m.ins[0].shape) == (2, cm, 8, 10) and tuple(got.shape) == (1, 16, 20, 2)
        G.assert_read(m.ins[0], gray, cm, 'model', 2, f'gray + alpha on {cm} channels')
        G.assert_written(got, m.outs[0][:1], m.outs[0][1:], f'gray + alpha from {cm} channels')
        if cm == 3:
            assert torch.equal(m.ins[0][:, 0], m.ins[0][:, 1]) and torch.equal(m.ins[0][:, 0], m.ins[0][:, 2])


def test_refusals():
    img = G.random_image(1, 24, 40, 4, 8, seed=1)
    up = tiling.upscale_rgba
    ran = _Fake(2)
    for bad in (torch.zeros(1, 4, 4, 5, dtype=torch.uint8), torch.zeros(4, 4, 0, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8),
                img.float(), img.to(torch.int32), img.double() / 255):  # fmt: skip
        with pytest.raises(ValueError):
            up(ran, bad, scale=2)
    for bad in (dict(bleed=17), dict(bleed=-1), dict(bleed=2.5), dict(out_bits=12), dict(out_bits=10), dict(alpha='premultiplied'), dict(resample='lanczos')):
        with pytest.raises(ValueError, match=list(bad)[0] if 'resample' not in bad else 'lanczos'):
            up(ran, img, scale=2, **bad)
    with pytest.raises(ValueError, match='gray'):
        up(_WithInfo(1, 1), img)  # a colour image on a one-channel model
    with pytest.raises(ValueError, match='gray'):
        up(_WithInfo(1, 1), img[..., :3])
    for cin, cout in ((3, 1), (1, 3), (4, 4), (2, 2)):
        with pytest.raises(ValueError, match='channels'):
            up(_WithInfo(cin, cout), img)
    assert up(_WithInfo(3, 3), img, dtype=torch.float32).shape == (1, 48, 80, 4)  # the scale comes from parameters_info
    with pytest.raises(ValueError, match='scale'):
        up(ran, img)
    with pytest.raises(ValueError, match='not both'):
        up(ran, img, scale=2, out_size=(10, 10), out_scale=2)
    with pytest.raises(ValueError, match='out_scale'):
        up(ran, img, scale=2, out_scale=0)
    with pytest.raises(ValueError, match='out_size'):
        up(ran, img, scale=2, out_size=(0, 10))
    with pytest.raises(ValueError, match='more than 8'):
        up(ran, img, scale=2, out_size=(4, 80))
    with pytest.raises(ValueError, match='blend'):
        up(ran, img, scale=2, blend=-1)
    assert not ran.ins  # every refusal came before the model ran
    with pytest.raises(ValueError, match='exceeds the halo'):
        up(ran, img, scale=2, tile=TILE, halo=4, blend=6)
    with pytest.raises(ValueError):
        ops.nchw_to_image_alpha(torch.zeros(1, 2, 6, 8), None, 3, 8)
    with pytest.raises(ValueError):
        ops.nchw_to_image_alpha(torch.zeros(1, 3, 6, 8), torch.zeros(1, 2, 6, 8), 4, 8)
    with pytest.raises(ValueError):
        ops.nchw_to_image_alpha(torch.zeros(1, 3, 6, 8), None, 3, 12)
    with pytest.raises(TypeError):
        ops.image_to_nchw_alpha(img, dtype=torch.float64)
    assert 'upscale_rgba' in resselt_amd.__all__ and 'upscale' in resselt_amd.__all__ and 'upscale_yuv' in resselt_amd.__all__


READ_ORDER = ['img', 'pitch', 'batch_stride', 'bits', 'batch', 'H', 'W', 'C', 'Cm', 'bleed', 'color', 'color_dtype', 'alpha', 'alpha_mode', 'flags', 'stream']
WRITE_ORDER = ['color', 'color_dtype', 'Cm', 'alpha', 'alpha_dtype', 'Ca', 'batch', 'H', 'W', 'C', 'bits', 'img', 'pitch', 'batch_stride', 'stream']


@pytest.mark.parametrize('name,order', [('rsa_image_to_nchw_alpha', READ_ORDER), ('rsa_nchw_to_image_alpha', WRITE_ORDER)])
def test_internal_rows_name_the_arguments_in_the_order_of_the_documented_prototypes(name, order):
    import os
    import re

    restype, params = L.INTERNAL[name]
    assert restype is C.c_int and [k for k, _ in params] == order
    for k, t in params:
        want = C.c_int64 if k in ('pitch', 'batch_stride') else C.c_void_p if k in ('img', 'color', 'alpha', 'flags', 'stream') else C.c_int32
        assert t is want, k
    assert name not in L.SIGNATURES and name not in L.EXTENSIONS  # no header declares it
    with open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), '..', 'csrc', 'rgba.hip')) as fh:
        text = fh.read()
    for where in (r'//\s+int ' + name, r'extern "C" int ' + name):  # the prototype in the head comment, and the definition
        proto = re.search(where + r'\(([^)]*)\)', text).group(1)
        assert [a.split()[-1].lstrip('*') for a in re.sub(r'\s*//\s*', ' ', proto).split(',')] == order, where


E_ARG, E_ALIGN = -1, -3
IMG, COL, ALPHA, FLAGS = 0x100000, 0x900000, 0xA00000, 0xB00000  # fake aligned addresses: every call below is refused before a launch


def _args(name, **over):
    a = dict(img=IMG, pitch=256, batch_stride=256 * 32, bits=8, batch=1, H=32, W=48, C=4, Cm=3, color=COL, color_dtype=L.F16, alpha=ALPHA, stream=None)
    a.update(dict(bleed=8, alpha_mode=1, flags=FLAGS) if name == 'rsa_image_to_nchw_alpha' else dict(alpha_dtype=L.F32, Ca=1))
    a.update(over)
    return [a[k] for k, _ in L.INTERNAL[name][1]]


COMMON = [
    (dict(img=None), E_ARG), (dict(color=None), E_ARG), (dict(C=0), E_ARG), (dict(C=5), E_ARG), (dict(bits=10), E_ARG), (dict(bits=12), E_ARG), (dict(bits=0), E_ARG),
    (dict(H=0), E_ARG), (dict(W=-2), E_ARG), (dict(batch=0), E_ARG), (dict(Cm=2), E_ARG), (dict(Cm=4), E_ARG), (dict(Cm=1), E_ARG), (dict(Cm=0), E_ARG),
    (dict(color_dtype=3), E_ARG), (dict(color_dtype=-1), E_ARG),
    (dict(pitch=191), E_ARG), (dict(bits=16), E_ARG),  # 16-bit RGBA rows are 384 bytes: a pitch of 256 is too small
    (dict(batch=2, batch_stride=256 * 31), E_ARG), (dict(batch=65536, batch_stride=256 * 32), E_ARG),
    (dict(bits=16, pitch=384, img=IMG + 1), E_ALIGN), (dict(bits=16, pitch=385), E_ALIGN), (dict(bits=16, pitch=384, batch=2, batch_stride=384 * 32 + 1), E_ALIGN),
    (dict(color=COL + 1), E_ALIGN), (dict(color=COL + 2, color_dtype=L.F32), E_ALIGN), (dict(color=COL + 1, color_dtype=L.BF16), E_ALIGN),
]  # fmt: skip
READ_ONLY = [
    (dict(bleed=17), E_ARG), (dict(bleed=-1), E_ARG), (dict(alpha_mode=3), E_ARG), (dict(alpha_mode=-1), E_ARG), (dict(alpha=None), E_ARG), (dict(flags=None), E_ARG),
    (dict(C=2, alpha=None, Cm=1), E_ARG), (dict(H=16 * 65535 + 1), E_ARG), (dict(flags=FLAGS + 2), E_ALIGN), (dict(alpha=ALPHA + 1), E_ALIGN),
    (dict(alpha=ALPHA + 2, alpha_mode=2), E_ALIGN),
]  # fmt: skip
WRITE_ONLY = [
    (dict(Ca=2), E_ARG), (dict(Ca=0), E_ARG), (dict(alpha_dtype=3), E_ARG), (dict(alpha_dtype=-1), E_ARG), (dict(H=4 * 65535 + 1), E_ARG),
    (dict(alpha=ALPHA + 2), E_ALIGN), (dict(alpha=ALPHA + 1, alpha_dtype=L.F16), E_ALIGN),
]  # fmt: skip


@pytest.mark.parametrize('name,over,status', [('rsa_image_to_nchw_alpha', o, s) for o, s in COMMON + READ_ONLY] + [('rsa_nchw_to_image_alpha', o, s) for o, s in COMMON + WRITE_ONLY])
def test_argument_checks_return_before_any_launch(name, over, status):
    lib = L.load()
    assert getattr(lib, name)(*_args(name, **over)) == status, over
    assert name.encode() in lib.rsa_last_error_string()
