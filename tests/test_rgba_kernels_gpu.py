"""``rsa_image_to_nchw_alpha`` and ``rsa_nchw_to_image_alpha`` (csrc/rgba.hip) alone, against the f64 definition (tests/rgba_reference.py).

The input kernel's tile is ``TW x TH`` = 64 x 16.  Every case (channels x depth x float dtype) walks widths 1, 2, TW - 1, TW, TW + 1 and
2 TW + 3 and heights 1, TH - 1, TH, TH + 1 and 2 TH + 1 (pairs, not the product), and one frame of 2 TW + 4 columns: a contiguous tensor whose
width is a multiple of 4 takes the kernel's vector path, every other size its element-wise path.  Patterns: random masks with half and with
99.9 % of the pixels transparent, a transparent hole ``2 bleed + 3`` wide that straddles the corner of the first tile (its centre keeps its
stored colour), a single known pixel at that corner, all opaque, all transparent; ``bleed`` 0, 1, 8 and 16; batch 1 and 2.  Each launch runs
twice (bit-identical) and its flags are compared with the definition's.  Pitched images run on both paths of each kernel, which must agree
bit for bit; the padding is poisoned, may not show in what is read and must be untouched by what is written.

Write tests use multiples of 1/64 in [-0.25, 1.25] (exact in f32, f16 and bf16) with one NaN pixel.  Bounds: rgba_reference.py."""

import functools

import pytest
import torch

import rgba_reference as G
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops

pytestmark = pytest.mark.gpu

TW, TH = 64, 16  # kRgbaTileW, kRgbaTileH
SIZES = [(1, 1), (TH - 1, 2), (TH, TW - 1), (TH + 1, TW), (2 * TH + 1, TW + 1), (TH + 1, 2 * TW + 3), (2 * TH + 1, 2 * TW + 4)]  # (H, W)
PATTERNS = {'half': (0, 1, 8, 16), 'sparse': (8, 16), 'hole': (1, 8, 16), 'single': (1, 16), 'opaque': (8,), 'transparent': (8,)}  # pattern -> bleeds
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
POISON = 0xA5


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _launches():
    """(H, W, pattern, bleed, N) of the launches of one case."""
    out = []
    for h, w in SIZES:
        for pattern, bleeds in PATTERNS.items():
            for bleed in bleeds:
                out.append((h, w, pattern, bleed, 1 + len(out) % 2))
    return out


def test_the_sizes_cover_what_they_claim():
    heights, widths = {h for h, _ in SIZES}, {w for _, w in SIZES}
    assert {1, TH - 1, TH, TH + 1, 2 * TH + 1} <= heights and {1, 2, TW - 1, TW, TW + 1, 2 * TW + 3} <= widths
    assert sum(w % 4 == 0 for w in widths) >= 2 and any(w % 4 == 0 and w > 2 * TW for w in widths)  # the vector path, past two tiles
    ls = _launches()
    assert {b for *_, b, _ in ls} == {0, 1, 8, 16} and {n for *_, n in ls} == {1, 2}
    for p, bleeds in PATTERNS.items():
        assert {(h, w) for h, w, pp, _, _ in ls if pp == p} == set(SIZES) and {b for _, _, pp, b, _ in ls if pp == p} == set(bleeds)


def _pattern(name: str, n: int, h: int, w: int, c: int, bits: int, bleed: int, seed: int) -> torch.Tensor:
    img = G.random_image(n, h, w, c, bits, seed, transparent={'sparse': 0.999}.get(name, 0.5))
    if not G.has_alpha(c) or name in ('half', 'sparse'):
        return img
    cy, cx = min(TH, h - 1), min(TW, w - 1)  # the corner the first four tiles share (clipped to a small image)
    if name == 'hole':
        return G.hole(img, cy, cx, 2 * bleed + 3)
    if name == 'single':
        return G.single_known(img, cy, cx)
    return G.with_alpha(img, G.DEPTHS[bits][1] if name == 'opaque' else 0)


@functools.lru_cache(maxsize=None)
def _read_case(i: int, c: int, bits: int):
    """(image, f64 colour, f64 alpha, flags) of launch ``i``: made once, shared by the destination dtypes and the alpha modes."""
    h, w, pattern, bleed, n = _launches()[i]
    img = _pattern(pattern, n, h, w, c, bits, bleed, seed=100 + i)
    return (img, *G.read64(img, bleed))


@pytest.mark.parametrize('c,bits,dst', [(4, 8, 'f16'), (4, 8, 'f32'), (4, 16, 'f32'), (4, 16, 'bf16'), (2, 8, 'bf16'), (2, 16, 'f16'), (3, 8, 'f16'), (3, 16, 'f32'), (1, 8, 'f32'), (1, 16, 'f16')])  # fmt: skip
def test_read_against_f64(device, c, bits, dst):
    dtype, worst, worst16 = DTYPES[dst], 0.0, 0.0
    for i, (h, w, pattern, bleed, n) in enumerate(_launches()):
        if not G.has_alpha(c) and (pattern not in ('half',) or bleed not in (0, 8)):
            continue  # images without alpha ignore the mask and the bleed
        img, col, a64, flags64 = _read_case(i, c, bits)
        cm = 3 if (c >= 3 or i % 3) else 1
        mode = ('model', 'resample')[i % 2]
        what = f'C={c} {bits} bits -> {dst} Cm={cm} {mode} {pattern} bleed {bleed} N={n} {h}x{w}'
        d = img.to(device)
        runs = [ops.image_to_nchw_alpha(d, cm, mode, bleed, dtype) for _ in range(2)]
        x, a, flags = runs[0]
        want = col.expand(n, cm, h, w) if col.shape[1] == 1 else col
        assert x.dtype == dtype and tuple(x.shape) == ((2 * n if (G.has_alpha(c) and mode == 'model') else n), cm, h, w), what
        ratio = ((x[:n].cpu().double() - want).abs() / G.read_bound(dtype, want, bleed if G.has_alpha(c) else 0)).max().item()
        assert ratio <= 1.0, f'{what}: {ratio:.3f} of the bound'
        worst = max(worst, ratio)
        if G.has_alpha(c) and bleed == 16 and dtype == torch.float32:  # the passes alone: error in units of 2^-24 where they ran longest
            worst16 = max(worst16, (x[:n].cpu().double() - want).abs().max().item() / G.U)
        if G.has_alpha(c):
            assert torch.equal(flags.cpu().bool(), flags64), f'{what}: flags {flags.tolist()}'
            got_a = x[n:].cpu().double() if mode == 'model' else a.cpu().double().expand(n, cm, h, w)
            assert bool(((got_a - a64.expand(n, cm, h, w)).abs() <= G.U + G.ROUNDING[dtype if mode == 'model' else torch.float32] * a64).all()), f'{what}: alpha'
            if pattern == 'hole' and h > TH and w > TW:  # the centre of the hole is bleed + 2 from the nearest known pixel
                stored = (G.codes_of(img)[:, : c - 1, TH, TW].float() / G.DEPTHS[bits][1]).to(dtype)  # [N, 1 or 3]: the f32 quotient a copy gives
                assert torch.equal(x[:n, :, TH, TW].cpu(), stored.expand(n, cm)), f'{what}: the centre of the hole moved'
        else:
            assert a is None and flags is None
        for t0, t1 in zip(runs[0], runs[1]):
            assert t0 is None or torch.equal(t0, t1), f'{what}: two runs differ'
    print(f'MEASURE read C={c} {bits} bits -> {dst}: worst error {worst:.3f} of its bound' + (f'; at bleed 16: {worst16:.2f} x 2^-24 of the allowed 129' if worst16 else ''))


# (H, W, extra pixels of a row, extra rows of an image): 4 extra pixels keep a width that is a multiple of 4 on the vector path, 1 or 3 leave it
PITCHED = [(5, 8, 4, 1), (TH + 2, TW + 4, 4, 2), (TH + 2, TW + 4, 1, 1), (2 * TH + 1, TW + 4, 3, 1), (TH + 1, TW + 3, 4, 2)]


def _padded(img: torch.Tensor, pad_w: int, pad_h: int) -> torch.Tensor:
    """``img`` ``[N, H, W, C]`` inside a poisoned buffer ``[N, H + pad_h, W + pad_w, C]`` (CPU)."""
    n, h, w, c = img.shape
    buf = torch.empty((n, h + pad_h, w + pad_w, c), dtype=img.dtype)
    buf.view(torch.uint8).fill_(POISON)
    buf[:, :h, :w].copy_(img)
    return buf


@pytest.mark.parametrize('c,bits', [(4, 8), (4, 16), (2, 8), (3, 8), (1, 16)])
def test_pitched_images_are_read_in_place_and_both_paths_agree(device, c, bits):
    n, bleed = 2, 8
    for h, w, pad_w, pad_h in PITCHED:
        img = G.random_image(n, h, w, c, bits, seed=h + w, transparent=0.9)
        view = _padded(img, pad_w, pad_h).to(device)[:, :h, :w]
        assert not view.is_contiguous() and ops._pitched_image(view)[0] is view
        for mode in ('model', 'resample'):
            got = ops.image_to_nchw_alpha(view, 3 if c >= 3 else 1, mode, bleed, torch.float32)
            ref = ops.image_to_nchw_alpha(img.to(device), 3 if c >= 3 else 1, mode, bleed, torch.float32)  # contiguous
            for g, r in zip(got, ref):
                assert (g is None and r is None) or torch.equal(g, r), f'C={c} {bits} bits {mode} {h}x{w} +{pad_w}: the pitched view reads differently'
            G.assert_read(got[0], img, 3 if c >= 3 else 1, mode, bleed, f'pitched read C={c} {bits} bits {mode} {h}x{w} +{pad_w}')


@pytest.mark.parametrize('c,bits', [(4, 8), (4, 16), (2, 16), (3, 8), (3, 16), (1, 8)])
def test_pitched_images_are_written_in_place_and_their_padding_is_untouched(device, c, bits):
    n, cm = 2, 3 if c >= 3 else 1
    dt, e = G.DEPTHS[bits][0], bits // 8
    for h, w, pad_w, pad_h in PITCHED:
        color = G.random_source(n, cm, h, w, seed=h * w).to(torch.float16).to(device)
        alpha = G.random_source(n, 1, h, w, seed=h * w + 1).to(device) if G.has_alpha(c) else None
        want = ops.nchw_to_image_alpha(color, alpha, c, bits).cpu()  # contiguous
        G.assert_written(want, color, alpha, f'write C={c} {bits} bits {h}x{w}')
        pitch = (w + pad_w) * c * e
        stride = pitch * (h + pad_h)
        buf = torch.full((n * stride,), POISON, dtype=torch.uint8, device=device)
        L.nchw_to_image_alpha(color.data_ptr(), L.F16, cm, None if alpha is None else alpha.data_ptr(), L.F32, 1, n, (h, w), c, bits,
                              (buf.data_ptr(), pitch, stride), ops.current_stream_ptr(device))  # fmt: skip
        got = buf.cpu().view(dt).reshape(n, h + pad_h, w + pad_w, c)
        assert torch.equal(got[:, :h, :w], want), f'C={c} {bits} bits {h}x{w} +{pad_w}: both paths of the kernel must agree'
        mask = torch.ones(got.shape, dtype=torch.bool)
        mask[:, :h, :w] = False
        assert bool((got.view(torch.uint8).reshape(*got.shape, e)[mask] == POISON).all()), f'C={c} {bits} bits {h}x{w} +{pad_w}: padding was written'


WRITE_SIZES = [(1, 1), (3, 5), (8, 12), (6, 10), (5, 260)]  # 12 and 260: multiples of the 4-pixel vector; 260: past one 256-column workgroup


@pytest.mark.parametrize('bits', [8, 16])
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_write_against_f64(device, c, bits):
    worst = -1.0
    for k, (h, w) in enumerate(WRITE_SIZES):
        n = 1 + k % 2
        for cm in ((1, 3) if c <= 2 else (3,)):
            color = G.random_source(n, cm, h, w, seed=300 + k + cm)
            for ca in (None, 1, cm) if G.has_alpha(c) else (None,):
                alpha = None if ca is None else G.random_source(n, ca, h, w, seed=400 + k + ca)
                target = G.write64(color, alpha, c, bits)
                for name, dtype in DTYPES.items():
                    xs, al = color.to(dtype), None if alpha is None else alpha.to(DTYPES['f32'] if name == 'f16' else dtype)  # a mixed pair too
                    assert torch.equal(xs.double().nan_to_num(7), color.double().nan_to_num(7)) and bool(xs.isnan().any())  # exact in every format
                    what = f'{name} Cm={cm} Ca={ca} -> C={c} {bits} bits N={n} {h}x{w}'
                    runs = [ops.nchw_to_image_alpha(xs.to(device), None if al is None else al.to(device), c, bits).cpu() for _ in range(2)]
                    assert runs[0].dtype == G.DEPTHS[bits][0] and tuple(runs[0].shape) == (n, h, w, c), what
                    err = G.code_error(runs[0], target)
                    assert err <= G.write_bound(bits), f'{what}: {err:.5f} codes > {G.write_bound(bits):.5f}'
                    assert torch.equal(runs[0].to(torch.int32), runs[1].to(torch.int32)), f'{what}: two runs differ'
                    if G.has_alpha(c) and ca is None:
                        assert set(runs[0][..., c - 1].to(torch.int32).flatten().tolist()) == {G.DEPTHS[bits][1]}, what
                    worst = max(worst, (err - 0.5) / (G.write_bound(bits) - 0.5))
    print(f'MEASURE write -> C={c} {bits} bits: worst (error - 0.5) / (bound - 0.5) = {worst:.3f}')


def test_refusals_and_cpu_dispatch(device):
    img = G.random_image(1, 6, 10, 4, 8, seed=2)
    with pytest.raises(ValueError, match='bleed'):
        ops.image_to_nchw_alpha(img.to(device), bleed=17)
    with pytest.raises(ValueError):
        ops.image_to_nchw_alpha(img.to(device), model_channels=1)
    with pytest.raises(RuntimeError, match='rsa_image_to_nchw_alpha'):
        L.image_to_nchw_alpha((img.to(device).data_ptr(), 39, 240), 8, 1, (6, 10), 4, 3, 8, 16, L.F16, 16, 1, 16, ops.current_stream_ptr(device))
    a = ops.image_to_nchw_alpha(img, 3, 'model', 8, torch.float32)  # CPU tensors: the torch form of the same definition
    b = ops.image_to_nchw_alpha(img.to(device), 3, 'model', 8, torch.float32)
    assert not a[0].is_cuda and (a[0] - b[0].cpu()).abs().max().item() <= 2 * (G.U + G.b_bleed(8)) and torch.equal(a[2], b[2].cpu())
