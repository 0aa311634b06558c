"""f64 reference of the video pixel formats of ``upscale_yuv``, written from the definition; it imports nothing of the code
under test.

A frame is a luma plane ``y`` ``[N, H, W]`` and a plane ``uv`` ``[N, H/2, W/2, 2]`` of interleaved (Cb, Cr) pairs: ``torch.uint8`` codes for
``bits = 8`` (NV12), ``torch.uint16`` words that hold the code in their top 10 bits for ``bits = 10`` (P010).  With ``m = 2^(bits - 8)``:

  limited range  ``Y' = (code - 16 m) / (219 m)``, ``Cb, Cr = (code - 128 m) / (224 m)``
  full range     ``Y' = code / (2^bits - 1)``, ``Cb, Cr = (code - 2^(bits - 1)) / (2^bits - 1)``
  matrix         ``R = Y' + 2 (1 - Kr) Cr``, ``B = Y' + 2 (1 - Kb) Cb``, ``G = (Y' - Kr R - Kb B) / Kg``; and back ``Y' = Kr R + Kg G + Kb B``,
                 ``Cb = (B - Y') / (2 (1 - Kb))``, ``Cr = (R - Y') / (2 (1 - Kr))``
  siting         chroma sample ``j`` of an axis sits at luma coordinate ``2 j + o``: 'left' has ``o = 0`` horizontally and ``0.5`` vertically,
                 'center' ``0.5`` on both axes
  read           luma coordinate ``x`` takes chroma position ``u = (x - o) / 2`` linearly from samples ``floor(u)`` and ``floor(u) + 1``
                 (indices clamped); R, G, B are clamped to [0, 1]
  write          the source is clamped to [0, 1] (NaN -> 0); Cb, Cr per luma pixel; an axis with ``o = 0.5`` takes the mean of luma positions
                 ``2 j, 2 j + 1``, one with ``o = 0`` ``[1 2 1] / 4`` over ``2 j - 1, 2 j, 2 j + 1`` (indices clamped); the code is the inverse
                 of the normalisation, rounded half to even and clamped to ``[0, 2^bits - 1]``

Bounds (derived, not measured).  Each path is at most 12 f32 operations on magnitudes below 2, each with a relative error of 2^-24, and the
constants are rounded to f32 once: ``B = 32 * 2^-24`` covers both.  A value read into f32 is within ``B`` of ``to_rgb64``, into f16 / bf16
within ``B + u |v|`` (u = 2^-11 / 2^-8: one rounding of the destination).  A written code is within ``0.5 + 2^bits * B`` of the UNROUNDED target
of ``to_yuv64`` (the factor 2^bits > 219 m, 224 m, 2^bits - 1 turns the error of the normalised value into codes; 0.5 is the rounding itself).
Comparing with the unrounded target makes ties harmless: whichever way a tie goes, the code is 0.5 from the target."""

import torch

MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722), 'bt2020': (0.2627, 0.0593)}
FORMATS = {'nv12': (8, torch.uint8), 'p010': (10, torch.uint16)}
RANGES = ('limited', 'full')
CHROMA_LOCS = ('left', 'center')
B = 32 * 2.0**-24
ROUNDING = {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}  # beyond f32, whose own rounding is one of B's operations


def _levels(bits: int, range: str):
    """(luma offset, luma range, chroma offset, chroma range) in codes."""
    m, top = 2 ** (bits - 8), 2**bits - 1
    if range == 'limited':
        return 16 * m, 219 * m, 128 * m, 224 * m
    assert range == 'full'
    return 0, top, 2 ** (bits - 1), top


def _offsets(chroma_loc: str):
    """(vertical, horizontal) siting offset o."""
    return {'left': (0.5, 0.0), 'center': (0.5, 0.5)}[chroma_loc]


def codes_of(plane: torch.Tensor, bits: int) -> torch.Tensor:
    """The codes of a plane as f64 (P010: the top 10 bits of each word)."""
    c = plane.to(torch.int64)
    return (c >> 6 if bits == 10 else c).to(torch.float64)


def _interp_axis(c: torch.Tensor, dim: int, n: int, o: float) -> torch.Tensor:
    out = []
    last = c.shape[dim] - 1
    for x in range(n):
        u = (x - o) / 2
        j = int(u // 1)
        f = u - j
        a, b = min(max(j, 0), last), min(max(j + 1, 0), last)
        out.append((1 - f) * c.select(dim, a) + f * c.select(dim, b))
    return torch.stack(out, dim)


def to_rgb64(y: torch.Tensor, uv: torch.Tensor, fmt: str = 'nv12', matrix: str = 'bt709', range: str = 'limited', chroma_loc: str = 'left') -> torch.Tensor:
    """Planes ``y`` ``[N, H, W]``, ``uv`` ``[N, H/2, W/2, 2]`` -> f64 ``[N, 3, H, W]`` R, G, B in [0, 1]."""
    bits, _ = FORMATS[fmt]
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    y_off, y_range, c_off, c_range = _levels(bits, range)
    oy, ox = _offsets(chroma_loc)
    n, h, w = y.shape
    yn = (codes_of(y, bits) - y_off) / y_range
    c = (codes_of(uv, bits) - c_off) / c_range
    c = _interp_axis(_interp_axis(c, 1, h, oy), 2, w, ox)
    cb, cr = c[..., 0], c[..., 1]
    r = yn + 2 * (1 - kr) * cr
    b = yn + 2 * (1 - kb) * cb
    g = (yn - kr * r - kb * b) / kg
    return torch.stack((r, g, b), 1).clamp(0, 1)


def _filter_axis(d: torch.Tensor, dim: int, o: float) -> torch.Tensor:
    n = d.shape[dim]
    out = []
    for j in range(n // 2):
        if o == 0.5:
            out.append((d.select(dim, 2 * j) + d.select(dim, 2 * j + 1)) / 2)
        else:
            out.append((d.select(dim, max(2 * j - 1, 0)) + 2 * d.select(dim, 2 * j) + d.select(dim, 2 * j + 1)) / 4)
    return torch.stack(out, dim)


def to_yuv64(rgb: torch.Tensor, fmt: str = 'nv12', matrix: str = 'bt709', range: str = 'limited', chroma_loc: str = 'left'):
    """``rgb`` ``[N, 3, H, W]`` (any float dtype; NaN counts as 0) -> the UNROUNDED code-valued targets ``(y [N, H, W], uv [N, H/2, W/2, 2])`` in
    f64, clamped to ``[0, 2^bits - 1]`` (rounding and clamping commute for integer limits)."""
    bits, _ = FORMATS[fmt]
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    y_off, y_range, c_off, c_range = _levels(bits, range)
    oy, ox = _offsets(chroma_loc)
    v = rgb.to(torch.float64)
    v = torch.where(v.isnan(), torch.zeros_like(v), v).clamp(0, 1)
    r, g, b = v[:, 0], v[:, 1], v[:, 2]
    yn = kr * r + kg * g + kb * b
    cb, cr = (b - yn) / (2 * (1 - kb)), (r - yn) / (2 * (1 - kr))
    c = _filter_axis(_filter_axis(torch.stack((cb, cr), -1), 1, oy), 2, ox)
    top = 2**bits - 1
    return (yn * y_range + y_off).clamp(0, top), (c * c_range + c_off).clamp(0, top)


def plane_error(got: torch.Tensor, target: torch.Tensor, bits: int) -> float:
    """Largest distance, in codes, of the plane ``got`` (uint8 codes, or uint16 P010 words) from the f64 ``target`` of ``to_yuv64``."""
    assert tuple(got.shape) == tuple(target.shape), (tuple(got.shape), tuple(target.shape))
    return (codes_of(got, bits) - target).abs().max().item()


def read_bound(dtype: torch.dtype, want: torch.Tensor) -> torch.Tensor:
    """Per element: what a value read into ``dtype`` may differ from ``want`` (f64, in [0, 1])."""
    return B + ROUNDING[dtype] * want.abs()


def write_bound(bits: int) -> float:
    return 0.5 + 2**bits * B


def low_bits(plane: torch.Tensor) -> torch.Tensor:
    """The 6 bits of each P010 word below the code."""
    return plane.to(torch.int64) & 63


def random_planes(n: int, h: int, w: int, fmt: str, seed: int):
    """Random codes over the whole range of the format (0 and the maximum included, both out of range for 'limited'), and for P010 random
    low bits, which a reader must ignore."""
    bits, dt = FORMATS[fmt]
    g = torch.Generator().manual_seed(seed)
    top = 2**bits - 1
    y = torch.randint(0, top + 1, (n, h, w), generator=g)
    uv = torch.randint(0, top + 1, (n, h // 2, w // 2, 2), generator=g)
    y.view(-1)[0], y.view(-1)[-1], uv.view(-1)[0], uv.view(-1)[-1] = 0, top, top, 0
    if bits == 10:
        y = (y << 6) | torch.randint(0, 64, y.shape, generator=g)
        uv = (uv << 6) | torch.randint(0, 64, uv.shape, generator=g)
    return y.to(torch.int32).to(dt), uv.to(torch.int32).to(dt)


def random_rgb(n: int, h: int, w: int, seed: int) -> torch.Tensor:
    """f32 ``[N, 3, H, W]`` of multiples of 1/64 in [-0.25, 1.25] (exact in f32, f16 and bf16), with one NaN pixel."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 81, (n, 3, h, w), generator=g).to(torch.float32) / 64
    x[0, :, h // 2, w // 2] = float('nan')
    return x


def assert_read(got: torch.Tensor, y: torch.Tensor, uv: torch.Tensor, what: str, **kw) -> None:
    """``got`` (what the model was given) is within the read bound of ``to_rgb64`` of the planes."""
    want = to_rgb64(y, uv, **kw)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f'{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}'
    ratio = ((got.double() - want).abs() / read_bound(got.dtype, want)).max().item()
    print(f'MEASURE {what}: read error {ratio:.3f} of its bound ({got.dtype})')
    assert ratio <= 1.0, f'{what}: read error {ratio:.3f} of its bound'


def assert_written(y: torch.Tensor, uv: torch.Tensor, rgb: torch.Tensor, what: str, extra: float = 0.0, **kw) -> None:
    """The planes ``y``, ``uv`` are within the write bound of ``to_yuv64`` of ``rgb``; ``extra`` is what ``rgb`` itself may be off (in
    normalised units: an error e of R, G, B moves Y' by at most e and Cb, Cr by at most e, so a code by less than 2^bits * e)."""
    bits, dt = FORMATS[kw.get('fmt', 'nv12')]
    ty, tuv = to_yuv64(rgb, **kw)
    y, uv = y.detach().cpu(), uv.detach().cpu()
    assert y.dtype == dt and uv.dtype == dt and y.is_contiguous() and uv.is_contiguous(), what
    if bits == 10:
        assert int(low_bits(y).max()) == 0 and int(low_bits(uv).max()) == 0, f'{what}: low bits of a P010 word are set'
    allowed = write_bound(bits) + 2**bits * extra
    err_y, err_c = plane_error(y, ty, bits), plane_error(uv, tuv, bits)
    print(f'MEASURE {what}: luma {err_y:.5f} codes, chroma {err_c:.5f} codes; (worst - 0.5) / (bound - 0.5) = {(max(err_y, err_c) - 0.5) / (allowed - 0.5):.3f}')
    assert max(err_y, err_c) <= allowed, f'{what}: {max(err_y, err_c):.5f} codes > {allowed:.5f}'
