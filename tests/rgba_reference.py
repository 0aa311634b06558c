"""f64 reference of the still-image formats of ``upscale_rgba``, written from the definition; it imports nothing of the code
under test.

An image is ``[N, H, W, C]`` of ``torch.uint8`` (``M = 255``) or ``torch.uint16`` (``M = 65535``, the full range): ``C`` = 1 gray, 2 gray +
alpha, 3 RGB, 4 RGBA; alpha is straight and is the last channel.

  read    value = code / M; gray is replicated to the model's ``Cm`` channels
  bleed   ``K_0 = {alpha code > 0}``.  Pass ``p = 1 .. bleed``: every pixel outside ``K_(p-1)`` whose 3 x 3 neighbours (centre and positions
          outside the image excluded) hold a non-empty set ``S`` of pixels of ``K_(p-1)`` takes ``sum_S w c_(p-1) / sum_S w`` (``w`` = 2 for the
          four edge neighbours, 1 for the four diagonal ones) and joins ``K_p``; every other pixel keeps its colour; alpha never changes
  write   gray = the mean of the ``Cm`` colour channels, alpha = the mean of the alpha source's channels (no source: 1); each value is clamped
          to [0, 1] (NaN -> 0), multiplied by ``M`` and rounded half to even

Bounds (derived, not measured), ``u = 2^-24`` (the relative error of one f32 operation):
  ``B_BLEED(r) = 8 r u``: one pass is a sum of at most 8 non-negative terms (7 additions, each with a relative rounding of a partial sum
    that is at most the total; the products by 2 and the sum of the weights are exact) and one division: at most 8 relative roundings of a
    value that is at most 1.  Later passes are convex combinations of earlier values and do not amplify their errors.  The kernel and the
    torch form divide by a true division, so no reciprocal's error is added.
  read: ``code / M`` is one division: ``u``.  A value read into f32 is within ``u + B_BLEED(bleed)`` of the f64 value (``u`` alone without an
    alpha channel), into f16 / bf16 within that plus ``U |v|`` (``U`` = 2^-11 / 2^-8: one rounding of the destination).
  ``B_OUT = 4 u``: the mean of three is two additions and a division, the scale by ``M`` one multiplication, each one rounding of a value
    that is at most 1 (times ``M``).  A written code is within ``0.5 + M B_OUT`` of the UNROUNDED f64 target (0.5 is the rounding itself;
    comparing with the unrounded target makes ties harmless)."""

import torch
import torch.nn.functional as F

U = 2.0**-24
B_OUT = 4 * U
ROUNDING = {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
DEPTHS = {8: (torch.uint8, 255), 16: (torch.uint16, 65535)}
_KERNEL = torch.tensor([[1.0, 2.0, 1.0], [2.0, 0.0, 2.0], [1.0, 2.0, 1.0]], dtype=torch.float64)


def b_bleed(passes: int) -> float:
    return 8 * passes * U


def bits_of(img: torch.Tensor) -> int:
    return {torch.uint8: 8, torch.uint16: 16}[img.dtype]


def has_alpha(c: int) -> bool:
    return c in (2, 4)


def codes_of(img: torch.Tensor) -> torch.Tensor:
    """int64 ``[N, C, H, W]`` codes of an ``[N, H, W, C]`` image."""
    return img.to(torch.int32).to(torch.int64).permute(0, 3, 1, 2)


def bleed64(col: torch.Tensor, known: torch.Tensor, passes: int):
    """``(colour, known)`` after ``passes`` passes: f64 ``col`` ``[N, Cs, H, W]``, bool ``known`` ``[N, 1, H, W]``."""
    k = _KERNEL.reshape(1, 1, 3, 3)
    for _ in range(passes):
        kf = known.to(torch.float64)
        den = F.conv2d(kf, k, padding=1)  # zero padding: positions outside the image are not in S
        num = torch.cat([F.conv2d(col[:, c : c + 1] * kf, k, padding=1) for c in range(col.shape[1])], 1)
        fill = ~known & (den > 0)
        col = torch.where(fill, num / den.clamp(min=1), col)
        known = known | fill
    return col, known


def read64(img: torch.Tensor, bleed: int):
    """``(colour f64 [N, Cs, H, W] after the bleed, alpha f64 [N, 1, H, W] or None, flags bool [N] or None)`` of an ``[N, H, W, C]`` image."""
    m = DEPTHS[bits_of(img)][1]
    codes = codes_of(img)
    c = codes.shape[1]
    col = codes[:, : c - has_alpha(c)].to(torch.float64) / m
    if not has_alpha(c):
        return col, None, None
    ac = codes[:, c - 1 :]
    col, _ = bleed64(col, ac > 0, bleed)
    return col, ac.to(torch.float64) / m, (ac.reshape(ac.shape[0], -1) < m).any(1)


def model_input64(img: torch.Tensor, cm: int, alpha: str, bleed: int):
    """What the model is given: f64 ``[N, Cm, H, W]`` colour, with ``alpha = 'model'`` on a translucent batch followed by the ``N`` alpha
    entries replicated to ``Cm`` channels."""
    col, a, flags = read64(img, bleed)
    n, _, h, w = col.shape
    x = col.expand(n, cm, h, w) if col.shape[1] == 1 else col
    if a is not None and alpha == 'model' and bool(flags.any()):
        x = torch.cat((x, a.expand(n, cm, h, w)))
    return x


def write64(color: torch.Tensor, alpha, c: int, bits: int) -> torch.Tensor:
    """The UNROUNDED f64 targets ``[N, H, W, C]``, in codes, of a colour tensor ``[N, Cm, H, W]`` and an alpha source ``[N, Ca, H, W]`` or None."""
    m = DEPTHS[bits][1]
    v = color.to(torch.float64)
    planes = [v.mean(1)] if c <= 2 else [v[:, i] for i in range(3)]
    if has_alpha(c):
        planes.append(alpha.to(torch.float64).mean(1) if alpha is not None else torch.ones_like(planes[0]))
    t = torch.stack(planes, -1)
    return torch.where(t.isnan(), torch.zeros_like(t), t).clamp(0, 1) * m


def read_bound(dtype: torch.dtype, want: torch.Tensor, bleed: int) -> torch.Tensor:
    return U + b_bleed(bleed) + ROUNDING[dtype] * want.abs()


def write_bound(bits: int, extra: float = 0.0) -> float:
    m = DEPTHS[bits][1]
    return 0.5 + m * (B_OUT + extra)


def assert_read(got: torch.Tensor, img: torch.Tensor, cm: int, alpha: str, bleed: int, what: str) -> float:
    """``got`` (what the model was given) is within the read bound of ``model_input64``; returns the worst error as a fraction of the bound."""
    c = img.shape[3]
    want = model_input64(img, cm, alpha, bleed)
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f'{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}'
    ratio = ((got.double() - want).abs() / read_bound(got.dtype, want, bleed if has_alpha(c) else 0)).max().item()
    print(f'MEASURE {what}: read error {ratio:.3f} of its bound ({got.dtype})')
    assert ratio <= 1.0, f'{what}: read error {ratio:.3f} of its bound'
    return ratio


def code_error(got: torch.Tensor, target: torch.Tensor) -> float:
    assert tuple(got.shape) == tuple(target.shape), (tuple(got.shape), tuple(target.shape))
    return (got.to(torch.int32).to(torch.float64) - target).abs().max().item()


def assert_written(got: torch.Tensor, color: torch.Tensor, alpha, what: str, extra: float = 0.0) -> float:
    """The image ``got`` is within the write bound of ``write64``; ``extra`` is what the sources themselves may be off (normalised units).
    Returns (worst - 0.5) / (bound - 0.5)."""
    got = got.detach().cpu()
    bits, c = bits_of(got), got.shape[3]
    assert got.is_contiguous(), what
    target = write64(color.detach().cpu(), None if alpha is None else alpha.detach().cpu(), c, bits)
    allowed, err = write_bound(bits, extra), code_error(got, target)
    ratio = (err - 0.5) / (allowed - 0.5)
    print(f'MEASURE {what}: {err:.5f} codes; (worst - 0.5) / (bound - 0.5) = {ratio:.3f}')
    assert err <= allowed, f'{what}: {err:.5f} codes > {allowed:.5f}'
    return ratio


def _to_image(codes: torch.Tensor, bits: int) -> torch.Tensor:
    return codes.to(torch.int32).to(DEPTHS[bits][0]).contiguous()


def random_image(n: int, h: int, w: int, c: int, bits: int, seed: int, transparent: float = 0.5) -> torch.Tensor:
    """Random codes over the whole range (0 and the maximum included); with an alpha channel a fraction ``transparent`` of the pixels has
    alpha 0 (their stored colour is random too), the others a random alpha in 1 .. maximum, a third of them the maximum itself."""
    g = torch.Generator().manual_seed(seed)
    m = DEPTHS[bits][1]
    codes = torch.randint(0, m + 1, (n, h, w, c), generator=g)
    codes.view(-1)[0] = 0
    codes.view(-1)[-1 - has_alpha(c)] = m
    if has_alpha(c):
        a = torch.randint(1, m + 1, (n, h, w), generator=g)
        a[torch.rand((n, h, w), generator=g) < 1 / 3] = m
        a[torch.rand((n, h, w), generator=g) < transparent] = 0
        codes[..., c - 1] = a
    return _to_image(codes, bits)


def with_alpha(img: torch.Tensor, alpha_codes: torch.Tensor) -> torch.Tensor:
    """``img`` with its alpha channel replaced by the codes ``alpha_codes`` ``[N, H, W]`` (or a number)."""
    codes = img.to(torch.int32).clone()
    codes[..., -1] = alpha_codes
    return codes.to(img.dtype).contiguous()


def hole(img: torch.Tensor, cy: int, cx: int, side: int) -> torch.Tensor:
    """Opaque everywhere but a transparent square of ``side`` pixels centred at ``(cy, cx)`` (clipped to the image)."""
    m = DEPTHS[bits_of(img)][1]
    a = torch.full(img.shape[:3], m, dtype=torch.int32)
    r = side // 2
    a[:, max(cy - r, 0) : cy + r + 1, max(cx - r, 0) : cx + r + 1] = 0
    return with_alpha(img, a)


def single_known(img: torch.Tensor, cy: int, cx: int) -> torch.Tensor:
    """Transparent everywhere but the pixel ``(cy, cx)``."""
    a = torch.zeros(img.shape[:3], dtype=torch.int32)
    a[:, cy, cx] = 1 + (cy + cx) % DEPTHS[bits_of(img)][1]
    return with_alpha(img, a)


def random_source(n: int, ch: int, h: int, w: int, seed: int) -> torch.Tensor:
    """f32 ``[N, ch, H, W]`` of multiples of 1/64 in [-0.25, 1.25] (exact in f32, f16 and bf16), with one NaN pixel."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 81, (n, ch, h, w), generator=g).to(torch.float32) / 64
    x[0, :, h // 2, w // 2] = float('nan')
    return x
