"""``rsa_yuv420_to_nchw`` and ``rsa_nchw_to_yuv420`` (csrc/yuv.hip) alone, against the f64 definition (tests/yuv_reference.py).

Every case (pixel format x float dtype) walks the same sizes with both chroma sitings and both ranges, the three matrices and batch 1 / 2
rotating: 2 x 2 (one chroma sample: every clamp at once), 2 x 34, 34 x 2, 6 x 10 and 4 x 26 (widths that are 2 mod 8), heights and widths two
below, at, two above and past twice the kernel's 16 x 256 workgroup tile, and two frames whose width is a multiple of 8 past one and two tiles:
the contiguous tensors of ``ops`` then take the kernel's vector path, every other size its element-wise path.  Pitched planes (a pitch larger
than the row, a batch stride larger than the image, poison in the padding) run on both paths.

Read tests use random codes over the whole range of the format (0 and the maximum are out of range for 'limited'; P010 words carry random
low bits), write tests multiples of 1/64 in [-0.25, 1.25] (exact in f32, f16 and bf16) with one NaN pixel.  Bounds: yuv_reference.py."""

import functools

import pytest
import torch

import yuv_reference as Y
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 16, 256  # kYuvTileH, kYuvTileW
SIZES = [(2, 2), (2, 34), (34, 2), (6, 10), (4, 26), (TILE_H - 2, TILE_W - 2), (TILE_H, TILE_W), (TILE_H + 2, TILE_W + 2), (2 * TILE_H + 2, 2 * TILE_W + 2),
         (TILE_H + 2, TILE_W + 8), (2 * TILE_H + 4, 2 * TILE_W + 8)]  # fmt: skip
MATRICES, BATCHES = tuple(Y.MATRICES), (1, 2)
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
POISON = 0xA5


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _launches():
    """(H, W, matrix, N, range, chroma_loc) of the launches of one case."""
    out = []
    for i, (h, w) in enumerate(SIZES):
        for r in Y.RANGES:
            for c in Y.CHROMA_LOCS:
                out.append((h, w, MATRICES[(i + len(out)) % 3], BATCHES[(i // 2 + len(out)) % 2], r, c))
    return out


def test_the_sizes_cover_what_they_claim():
    heights, widths = {h for h, _ in SIZES}, {w for _, w in SIZES}
    assert {TILE_H - 2, TILE_H, TILE_H + 2} <= heights and max(heights) > 2 * TILE_H
    assert {TILE_W - 2, TILE_W, TILE_W + 2} <= widths and max(widths) > 2 * TILE_W
    assert (2, 2) in SIZES and (2, 34) in SIZES and (34, 2) in SIZES and (6, 10) in SIZES and sum(w % 8 == 2 for w in widths) >= 3
    assert any(w % 8 == 0 and w > TILE_W for w in widths) and any(w % 8 == 0 and w > 2 * TILE_W for w in widths)  # the vector path, past a tile
    ls = _launches()
    assert {(m, n) for _, _, m, n, _, _ in ls} == {(m, n) for m in MATRICES for n in BATCHES}
    for h, w in SIZES:
        assert {(r, c) for hh, ww, _, _, r, c in ls if (hh, ww) == (h, w)} == {(r, c) for r in Y.RANGES for c in Y.CHROMA_LOCS}


@functools.lru_cache(maxsize=None)
def _read_case(i: int, fmt: str):
    """(planes, f64 reference) of launch ``i``: made once, shared by the three destination dtypes."""
    h, w, matrix, n, r, c = _launches()[i]
    y, uv = Y.random_planes(n, h, w, fmt, seed=100 + i)
    return y, uv, Y.to_rgb64(y, uv, fmt, matrix, r, c)


@functools.lru_cache(maxsize=None)
def _write_case(i: int, fmt: str):
    """(f32 source, unrounded f64 targets) of launch ``i``: the source is exact in every float dtype, so one reference serves all three."""
    h, w, matrix, n, r, c = _launches()[i]
    x = Y.random_rgb(n, h, w, seed=300 + i)
    return x, Y.to_yuv64(x, fmt, matrix, r, c)


@pytest.mark.parametrize('dst', list(DTYPES))
@pytest.mark.parametrize('fmt', list(Y.FORMATS))
def test_read_against_f64(device, fmt, dst):
    dtype, worst = DTYPES[dst], 0.0
    for i, (h, w, matrix, n, r, c) in enumerate(_launches()):
        y, uv, want = _read_case(i, fmt)
        what = f'{fmt}->{dst} {matrix} {r} {c} N={n} {h}x{w}'
        yd, uvd = y.to(device), uv.to(device)
        runs = [ops.yuv420_to_nchw(yd, uvd, fmt, matrix, r, c, dtype).cpu() for _ in range(2)]
        assert runs[0].dtype == dtype and tuple(runs[0].shape) == (n, 3, h, w), what
        ratio = ((runs[0].double() - want).abs() / Y.read_bound(dtype, want)).max().item()
        assert ratio <= 1.0, f'{what}: {ratio:.3f} of the bound'
        assert torch.equal(runs[0], runs[1]), f'{what}: two runs differ'
        worst = max(worst, ratio)
    print(f'MEASURE read {fmt}->{dst}: worst error {worst:.3f} of its bound over {len(_launches())} launches')


@pytest.mark.parametrize('src', list(DTYPES))
@pytest.mark.parametrize('fmt', list(Y.FORMATS))
def test_write_against_f64(device, fmt, src):
    bits, dt = Y.FORMATS[fmt]
    allowed, worst = Y.write_bound(bits), 0.0
    for i, (h, w, matrix, n, r, c) in enumerate(_launches()):
        x, (ty, tuv) = _write_case(i, fmt)
        xs = x.to(DTYPES[src])
        assert torch.equal(xs.double().nan_to_num(7), x.double().nan_to_num(7)) and bool(xs.isnan().any())  # exact in every format; one NaN pixel
        what = f'{src}->{fmt} {matrix} {r} {c} N={n} {h}x{w}'
        xd = xs.to(device)
        runs = [tuple(t.cpu() for t in ops.nchw_to_yuv420(xd, fmt, matrix, r, c)) for _ in range(2)]
        gy, guv = runs[0]
        assert gy.dtype == dt and guv.dtype == dt and tuple(gy.shape) == (n, h, w) and tuple(guv.shape) == (n, h // 2, w // 2, 2), what
        if bits == 10:
            assert int(Y.low_bits(gy).max()) == 0 and int(Y.low_bits(guv).max()) == 0, f'{what}: low bits of a P010 word are set'
        err = max(Y.plane_error(gy, ty, bits), Y.plane_error(guv, tuv, bits))
        assert err <= allowed, f'{what}: {err:.5f} codes > {allowed:.5f}'
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f'{what}: two runs differ'
        worst = max(worst, (err - 0.5) / (allowed - 0.5))
    print(f'MEASURE write {src}->{fmt}: worst (error - 0.5) / (bound - 0.5) = {worst:.3f} over {len(_launches())} launches')


# (H, W, extra samples of a row, extra rows of an image): W = 264 with a pitch of 16 more samples stays on the vector path, the others leave it
PITCHED = [(6, 10, 3, 1), (18, 264, 16, 2), (18, 264, 5, 1), (34, 258, 6, 3)]


def _padded(plane: torch.Tensor, pad_w: int, pad_h: int):
    """``plane`` ``[N, rows, samples]`` inside a poisoned buffer ``[N, rows + pad_h, samples + pad_w]`` (CPU)."""
    n, rows, cols = plane.shape
    buf = torch.empty((n, rows + pad_h, cols + pad_w), dtype=plane.dtype)
    buf.view(torch.uint8).fill_(POISON)
    buf[:, :rows, :cols].copy_(plane)
    return buf


@pytest.mark.parametrize('h,w,pad_w,pad_h', PITCHED)
@pytest.mark.parametrize('fmt', list(Y.FORMATS))
def test_pitched_planes_are_read_in_place_and_their_padding_is_ignored(device, fmt, h, w, pad_w, pad_h):
    n, kw = 2, dict(fmt=fmt, matrix='bt709', range='limited', chroma_loc='left')
    y, uv = Y.random_planes(n, h, w, fmt, seed=h + w)
    yb = _padded(y, pad_w, pad_h).to(device)
    uvb = _padded(uv.reshape(n, h // 2, w), 2 * pad_w, pad_h).to(device)
    yv, uvv = yb[:, :h, :w], uvb[:, : h // 2, :w].unflatten(2, (w // 2, 2))
    assert not yv.is_contiguous() and not uvv.is_contiguous() and yv.stride(0) > h * yv.stride(1) and ops._pitched(yv, 1)[0] is yv and ops._pitched(uvv, 2)[0] is uvv
    for chroma_loc in Y.CHROMA_LOCS:
        kw['chroma_loc'] = chroma_loc
        got = ops.yuv420_to_nchw(yv, uvv, dtype=torch.float32, **kw).cpu()
        Y.assert_read(got, y, uv, f'pitched read {fmt} {chroma_loc} {h}x{w} +{pad_w}', **kw)
        assert torch.equal(got, ops.yuv420_to_nchw(y.to(device), uv.to(device), dtype=torch.float32, **kw).cpu())  # both paths of the kernel agree


@pytest.mark.parametrize('h,w,pad_w,pad_h', PITCHED)
@pytest.mark.parametrize('fmt', list(Y.FORMATS))
def test_pitched_planes_are_written_in_place_and_their_padding_is_untouched(device, fmt, h, w, pad_w, pad_h):
    n = 2
    bits, dt = Y.FORMATS[fmt]
    e = 1 if bits == 8 else 2
    x = Y.random_rgb(n, h, w, seed=h * w).to(torch.float16).to(device)
    y_pitch, uv_pitch = (w + pad_w) * e, (w + 2 * pad_w) * e
    y_stride, uv_stride = y_pitch * (h + pad_h), uv_pitch * (h // 2 + pad_h)
    for chroma_loc in Y.CHROMA_LOCS:
        yb = torch.full((n * y_stride,), POISON, dtype=torch.uint8, device=device)
        uvb = torch.full((n * uv_stride,), POISON, dtype=torch.uint8, device=device)
        L.nchw_to_yuv420(x.data_ptr(), L.F16, n, (h, w), ops.YUV_MATRICES['bt601'], 1, ops.YUV_CHROMA_LOCS[chroma_loc], bits, (yb.data_ptr(), y_pitch, y_stride),
                         (uvb.data_ptr(), uv_pitch, uv_stride), ops.current_stream_ptr(device))  # fmt: skip
        wy, wuv = (t.cpu() for t in ops.nchw_to_yuv420(x, fmt, 'bt601', 'full', chroma_loc))
        gy = yb.cpu().view(dt).reshape(n, h + pad_h, w + pad_w)
        guv = uvb.cpu().view(dt).reshape(n, h // 2 + pad_h, w + 2 * pad_w)
        assert torch.equal(gy[:, :h, :w], wy) and torch.equal(guv[:, : h // 2, :w], wuv.reshape(n, h // 2, w))  # both paths of the kernel agree
        Y.assert_written(wy, wuv, x.cpu(), f'pitched write {fmt} {chroma_loc} {h}x{w} +{pad_w}', fmt=fmt, matrix='bt601', range='full', chroma_loc=chroma_loc)
        for buf, rows, cols in ((gy, h, w), (guv, h // 2, w)):  # everything outside what was to be written must still be poison
            mask = torch.ones(buf.shape, dtype=torch.bool)
            mask[:, :rows, :cols] = False
            assert bool((buf.view(torch.uint8).reshape(*buf.shape, e)[mask] == POISON).all()), f'{fmt} {chroma_loc} {h}x{w}: padding was written'


def test_refusals_and_cpu_dispatch(device):
    y, uv = Y.random_planes(1, 6, 10, 'nv12', seed=2)
    with pytest.raises(ValueError, match='i420'):
        ops.yuv420_to_nchw(y.to(device), uv.to(device), 'i420')
    with pytest.raises(ValueError):
        ops.yuv420_to_nchw(y.to(device), uv.to(device), 'p010')
    with pytest.raises(RuntimeError, match='rsa_nchw_to_yuv420'):
        L.nchw_to_yuv420(y.to(device).data_ptr(), L.F16, 1, (5, 10), 0, 0, 0, 8, (1, 10, 60), (2, 10, 30), ops.current_stream_ptr(device))
    a = ops.yuv420_to_nchw(y, uv, dtype=torch.float32)  # CPU tensors: the torch form of the same definition
    b = ops.yuv420_to_nchw(y.to(device), uv.to(device), dtype=torch.float32).cpu()
    assert not a.is_cuda and (a - b).abs().max().item() <= 2 * Y.B
