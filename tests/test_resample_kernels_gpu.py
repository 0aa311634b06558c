"""``rsa_resample`` (csrc/resample.hip) alone, against torch's f64 antialiased interpolation of the exact source values.

Every case (source format x destination format) walks the same 38 launches: 19 size pairs, each with both filters, with C and N rotating
through 1, 3, 4, 5 and 1, 2.  The size pairs are those of tests/test_resample.py (non-integer shrinks, the ratio limit, enlargement,
identity, a 1 x 1 output, one axis kept), output heights and widths one below, at and one above the kernel's 16 x 64 output tile and past
two tiles, source rows whose length is no multiple of 4, and 7 x 5 -> 3 x 2, whose only band is clipped at both borders at once.

Float sources hold multiples of 1/64 in [-0.25, 1.25]: exact in f32, f16 and bf16, so one f64 reference per launch serves all three (and
the 8-bit source has its own).  The expected value is ``F.interpolate(..., antialias=True)`` in f64; test_resample.py pins the tables to it.

Tolerance: ``B = (T_h + T_w + 4) * 2^-24 * S_h * S_w * max(1, |x|max)`` computed from the launch's tables (tests/resample_reference.py), plus
one rounding of the destination format, ``u * |v|`` with u = 2^-24 / 2^-11 / 2^-8 for f32 / f16 / bf16 (and 2^-25 for f16's subnormals);
8-bit destinations are within ``0.5 + 255 * B`` of ``255 * clamp(v, 0, 1)``.  Two runs of a launch are bit-identical."""

import functools

import pytest
import torch

import resample_reference as R
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.tiling import resample_table, resample_tables_device

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 16, 64  # kResampleTileH, kResampleTileW
SIZE_PAIRS = [
    ((24, 40), (9, 13)), ((37, 29), (5, 4)), ((64, 64), (8, 8)), ((16, 20), (24, 50)), ((8, 8), (8, 8)), ((8, 5), (1, 1)), ((12, 20), (12, 7)),
    ((9, 14), (23, 14)),  # tests/test_resample.py
    ((20, 70), (15, 63)), ((20, 70), (16, 64)), ((20, 70), (17, 65)),  # around one output tile, shrinking
    ((9, 31), (15, 63)), ((9, 31), (16, 64)), ((9, 31), (17, 65)),  # ... enlarging
    ((70, 150), (33, 129)), ((130, 260), (17, 33)), ((5, 130), (40, 130)),  # three tiles per axis; the ratio limit over several tiles; columns kept
    ((7, 5), (3, 2)), ((33, 1030), (5, 129)),  # a band clipped at both borders; ratio 7.98 along a long row
]  # fmt: skip
CHANNELS, BATCHES, FILTERS = (1, 3, 4, 5), (1, 2), ('bicubic', 'bilinear')
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16, 'u8': torch.uint8}
ROUNDING = {'f32': 2.0**-24, 'f16': 2.0**-11, 'bf16': 2.0**-8}


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _launches():
    """(src size, dst size, C, N, filter) of the 38 launches of one case."""
    out = []
    for i, (src, dst) in enumerate(SIZE_PAIRS):
        for filter in FILTERS:
            out.append((src, dst, CHANNELS[i % 4], BATCHES[(i // 4) % 2], filter))
    return out


def test_the_launches_cover_what_they_claim():
    ls = _launches()
    assert len(ls) == 38 and {(c, n, f) for _, _, c, n, f in ls} == {(c, n, f) for c in CHANNELS for n in BATCHES for f in FILTERS}
    heights, widths = {d[0] for _, d, *_ in ls}, {d[1] for _, d, *_ in ls}
    assert {TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1} <= heights and {TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1} <= widths
    assert any(s[1] % 4 for s, *_ in ls) and ((7, 5), (3, 2)) in {(s, d) for s, d, *_ in ls}
    assert max(max(s[0] / d[0], s[1] / d[1]) for s, d, *_ in ls) == 8 and any(s[0] < d[0] for s, d, *_ in ls)
    assert max(resample_table(s[k], d[k], 'bicubic')[1].shape[1] for s, d, *_ in ls for k in (0, 1)) == 32  # one below the cap of 33 taps


@functools.lru_cache(maxsize=None)
def _case(i: int, u8: bool):
    """(source as f32 NCHW or uint8 NHWC, f64 reference, bound B) of launch ``i``: made once, shared by every format that can share it."""
    src, dst, c, n, filter = _launches()[i]
    g = torch.Generator().manual_seed(500 + i)
    if u8:
        x = torch.randint(0, 256, (n, *src, c), generator=g, dtype=torch.uint8)
        x64 = R.image_as_f64(x)
    else:
        x = torch.randint(-16, 81, (n, c, *src), generator=g).to(torch.float32) / 64
        x64 = x.double()
    ty, tx = resample_table(src[0], dst[0], filter), resample_table(src[1], dst[1], filter)
    return x, R.interpolate64(x64, dst, filter), R.bound(ty, tx, x64.abs().max().item())


@pytest.mark.parametrize('dst_fmt', list(DTYPES))
@pytest.mark.parametrize('src_fmt', list(DTYPES))
def test_resample_against_f64(device, src_fmt, dst_fmt):
    worst = 0.0
    for i, (src, dst, c, n, filter) in enumerate(_launches()):
        x, want, b = _case(i, src_fmt == 'u8')
        xs = x.to(DTYPES[src_fmt])
        assert torch.equal(xs.double(), x.double())  # the source values are exact in every format
        xd = xs.to(device)
        what = f'{src_fmt}->{dst_fmt} {filter} C={c} N={n} {src}->{dst}'
        if dst_fmt == 'u8':
            runs = [ops.resample_to_image_u8(xd, dst, filter).cpu() for _ in range(2)]
            assert runs[0].dtype == torch.uint8 and tuple(runs[0].shape) == (n, *dst, c), what
            err, allowed = R.image_error(runs[0], want), 0.5 + 255 * b
            assert err <= allowed, f'{what}: {err:.5f} codes > {allowed:.5f}'
            worst = max(worst, (err - 0.5) / (255 * b))
        else:
            runs = [ops.resample(xd, dst, filter, DTYPES[dst_fmt]).cpu() for _ in range(2)]
            assert runs[0].dtype == DTYPES[dst_fmt] and tuple(runs[0].shape) == (n, c, *dst), what
            diff = (runs[0].double() - want).abs()
            over = diff - (ROUNDING[dst_fmt] * want.abs() + 2.0**-25)  # what is left after the destination's one rounding
            assert bool((over <= b).all()), f'{what}: {over.max().item():.3e} beyond the rounding > B = {b:.3e}'
            worst = max(worst, (diff.max().item() if dst_fmt == 'f32' else over.max().item()) / b)
        assert torch.equal(runs[0], runs[1]), f'{what}: two runs differ'
    print(f'MEASURE resample {src_fmt}->{dst_fmt}: worst error {worst:.3f} of B over {len(_launches())} launches')


def test_default_dtypes_and_refusals(device):
    x = torch.rand(1, 3, 20, 30, device=device)
    assert ops.resample(x.half(), (10, 10)).dtype == torch.float16 and ops.resample(x, (10, 10), 'bilinear').dtype == torch.float32
    img = (x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert ops.resample(img, (10, 10)).dtype == torch.float32 and tuple(ops.resample(img, (10, 10)).shape) == (1, 3, 10, 10)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        ops.resample(x.cpu(), (10, 10))
    with pytest.raises(ValueError, match='more than 8'):
        ops.resample(x, (2, 10))
    with pytest.raises(ValueError, match='lanczos'):
        ops.resample_to_image_u8(x, (10, 10), 'lanczos')
    with pytest.raises(TypeError):
        ops.resample(x, (10, 10), dtype=torch.float64)


@pytest.mark.parametrize('src,dst', [((7, 5), (3, 2)), ((20, 70), (17, 65)), ((9, 31), (15, 63)), ((64, 64), (8, 8))])
@pytest.mark.parametrize('fmt', ['f32', 'u8'])
def test_nothing_is_written_outside_the_destination(device, fmt, src, dst):
    """The entry point itself, on a destination that lies inside a larger buffer of sentinels."""
    n, c, pad = 2, 3, 4096
    x = torch.rand((n, c, *src), generator=torch.Generator().manual_seed(3)).to(device)
    count = n * c * dst[0] * dst[1]
    dtype = DTYPES[fmt]
    sentinel = 77 if fmt == 'u8' else -123.0
    buf = torch.full((count + 2 * pad,), sentinel, dtype=dtype, device=device)
    (sy, wy), (sx, wx) = resample_tables_device(src[0], dst[0], 'bicubic', device), resample_tables_device(src[1], dst[1], 'bicubic', device)
    L.resample(x.data_ptr(), L.F32, n, c, src, buf.data_ptr() + pad * buf.element_size(), ops.rsa_dtype(dtype), dst, (sy.data_ptr(), wy.data_ptr(), wy.shape[1]),
               (sx.data_ptr(), wx.data_ptr(), wx.shape[1]), ops.current_stream_ptr(device))  # fmt: skip
    got = buf.cpu()
    assert bool((got[:pad] == sentinel).all()) and bool((got[pad + count :] == sentinel).all())
    want = ops.resample_to_image_u8(x, dst) if fmt == 'u8' else ops.resample(x, dst)
    assert torch.equal(got[pad : pad + count], want.cpu().reshape(-1))
