"""Tile-parallel whole-image inference.

The reference has no tiler and no distributed code; every SR model in scope is translation-equivariant up to its
receptive field, so an image shards into independent *input* tiles (3 channels: tiny) that are widened by a halo,
upscaled independently and cropped.  No activation ever crosses a GPU boundary; the only collective is the final
reassembly: an all-gather of equal-sized (padded) output tiles over RCCL/xGMI (``torch.distributed`` backend "nccl"
on ROCm), after which every rank holds the whole upscaled image.

Host logic only: works with any callable ``model(x) -> y`` (the CPU tests drive it with the oracle over gloo).
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Callable, Sequence

import torch


@dataclass(frozen=True)
class Tile:
    """One work item in input-pixel coordinates. ``y0:y1, x0:x1`` is the region this tile OWNS in the output grid;
    ``ry0:ry1, rx0:rx1`` is what it reads (owned region + halo, clamped to the image)."""

    index: int
    y0: int
    y1: int
    x0: int
    x1: int
    ry0: int
    ry1: int
    rx0: int
    rx1: int

    @property
    def shape(self) -> tuple[int, int]:
        return self.y1 - self.y0, self.x1 - self.x0


def _splits(total: int, parts: int, align: int) -> list[int]:
    """Boundaries of at most `parts` near-equal chunks of [0, total), interior boundaries rounded to `align`.
    A dimension too small for `parts` aligned chunks yields fewer (never an empty chunk)."""
    edges = [0]
    for i in range(1, parts):
        e = round(total * i / parts / align) * align
        if edges[-1] < e < total:
            edges.append(e)
    edges.append(total)
    return edges


def choose_grid(n_tiles: int, height: int, width: int) -> tuple[int, int]:
    """rows x cols = n_tiles with tile aspect closest to square (e.g. 8 tiles of a 16:9 frame -> 2 x 4)."""
    best = None
    for rows in range(1, n_tiles + 1):
        if n_tiles % rows:
            continue
        cols = n_tiles // rows
        th, tw = height / rows, width / cols
        score = max(th / tw, tw / th)
        if best is None or score < best[0]:
            best = (score, rows, cols)
    return best[1], best[2]


def plan_tiles(height: int, width: int, rows: int, cols: int, halo: int = 32, align: int = 1) -> list[Tile]:
    """Partition an H x W input into rows x cols tiles.  ``align`` keeps interior tile edges AND halo-extended read
    windows on multiples of e.g. the SwinIR window, so window partitions of a tile coincide with the full frame's."""
    if rows < 1 or cols < 1 or halo < 0 or align < 1:
        raise ValueError('rows, cols >= 1, halo >= 0, align >= 1 required')
    if halo % align:
        halo = (halo // align + 1) * align
    ys, xs = _splits(height, rows, align), _splits(width, cols, align)
    tiles = []
    for r in range(len(ys) - 1):
        for c in range(len(xs) - 1):
            y0, y1, x0, x1 = ys[r], ys[r + 1], xs[c], xs[c + 1]
            tiles.append(Tile(len(tiles), y0, y1, x0, x1, max(y0 - halo, 0), min(y1 + halo, height), max(x0 - halo, 0), min(x1 + halo, width)))
    return tiles


def _is_image(x: torch.Tensor) -> bool:
    """uint8 [N, H, W, C] images (what a decoder delivers; models with ``supports_u8`` read and write them) vs float [N, C, H, W] tensors."""
    return x.dtype == torch.uint8


def _finish(y: torch.Tensor) -> torch.Tensor:
    """Last step of every helper that hands an image back to the user: synchronise and ask the engine whether any kernel reported a
    failed hand-off (``EngineModule.forward`` itself never synchronises, so a failure of the LAST launches would otherwise surface one
    call late).  A no-op for CPU tensors (the CPU tests drive this module with the oracle)."""
    if isinstance(y, torch.Tensor) and y.is_cuda:
        from .engine import lib as L

        torch.cuda.synchronize(y.device)
        L.check_status('upscale')
    return y


def run_tile(model: Callable[[torch.Tensor], torch.Tensor], x: torch.Tensor, tile: Tile, scale: int) -> torch.Tensor:
    """Upscale one tile (with its halo) and crop the halo off the result (a view of the model's output, not a copy)."""
    img = _is_image(x)
    if tile.y1 <= tile.y0 or tile.x1 <= tile.x0:
        return x.new_zeros((x.shape[0], 0, 0, x.shape[3]) if img else (x.shape[0], x.shape[1], 0, 0))
    crop = (x[:, tile.ry0 : tile.ry1, tile.rx0 : tile.rx1] if img else x[:, :, tile.ry0 : tile.ry1, tile.rx0 : tile.rx1]).contiguous()
    y = model(crop)
    oy, ox = (tile.y0 - tile.ry0) * scale, (tile.x0 - tile.rx0) * scale
    th, tw = tile.shape
    return y[:, oy : oy + th * scale, ox : ox + tw * scale] if img else y[:, :, oy : oy + th * scale, ox : ox + tw * scale]


def warn_global_statistics(model, n_tiles: int) -> None:
    """Models whose class sets ``global_statistics`` (RealPLKSR: GroupNorm over the whole image) compute different statistics on every
    tile, so a tiled result depends on the tile size; the reference has no tiling and defines the whole-image result."""
    if n_tiles > 1 and getattr(model, 'global_statistics', False):
        import warnings

        warnings.warn(f'{type(model).__name__} normalises over the whole image: with {n_tiles} tiles every tile uses its own statistics and the '
                      'output differs from the untiled one', RuntimeWarning, stacklevel=3)  # fmt: skip


def blend_window(tile: Tile, height: int, width: int, blend: int, scale: int) -> tuple[int, int, int, int, int, int, int, int]:
    """What ``tile`` contributes to the blended output of a ``height`` x ``width`` input, in OUTPUT pixels:
    ``(py0, py1, px0, px1, ramp_top, ramp_bottom, ramp_left, ramp_right)``.

    Per axis a tile that owns input pixels ``[a0, a1)`` contributes ``[a0*s - B, a1*s + B)`` with ``B = blend * scale``, without the
    ``-B`` at ``a0 = 0`` and the ``+B`` at ``a1 = size`` (an image border has no neighbour).  At an interior edge the first (last) ``2B``
    pixels of that range are a rising (falling) ramp, ``u = (p - (edge*s - B) + 0.5) / (2B)`` and ``1 - u``, which the neighbour across
    the edge evaluates on the same pixels, so the two weights sum to one; everywhere else the weight is 1.  A ramp width of 0 means no
    ramp on that side."""
    b = blend * scale

    def axis(a0, a1, size):
        lo, hi = a0 > 0, a1 < size
        return a0 * scale - (b if lo else 0), a1 * scale + (b if hi else 0), (2 * b if lo else 0), (2 * b if hi else 0)

    py0, py1, top, bottom = axis(tile.y0, tile.y1, height)
    px0, px1, left, right = axis(tile.x0, tile.x1, width)
    return py0, py1, px0, px1, top, bottom, left, right


def _check_blend(tiles: Sequence[Tile], blend: int, halo: int, align: int) -> None:
    """The refusals of ``upscale_tiled(blend=)`` for a plan of more than one tile."""
    if halo % align:
        halo = (halo // align + 1) * align  # what plan_tiles made of it
    if blend > halo:
        raise ValueError(f'blend = {blend} exceeds the halo of {halo} pixels: a tile can only contribute what it has computed')
    for axis, lo, hi in (('rows', 'y0', 'y1'), ('columns', 'x0', 'x1')):
        spans = {(getattr(t, lo), getattr(t, hi)) for t in tiles}
        if len(spans) > 1:
            a0, a1 = min(spans, key=lambda s: s[1] - s[0])
            if 2 * blend > a1 - a0:
                raise ValueError(f'2 * blend = {2 * blend} exceeds the tile extent of {a1 - a0} pixels ({axis} {a0}:{a1}): the bands of adjacent seams would overlap')


def _ramp(length: int, rise: int, fall: int, device) -> torch.Tensor:
    """f32 weights of one axis of a contributed window: rising ramp of ``rise`` pixels, ones, falling ramp of ``fall`` pixels."""
    wgt = torch.ones(length, dtype=torch.float32, device=device)
    if rise:
        wgt[:rise] = (torch.arange(rise, dtype=torch.float32, device=device) + 0.5) / rise
    if fall:
        wgt[length - fall :] *= 1 - (torch.arange(fall, dtype=torch.float32, device=device) + 0.5) / fall
    return wgt


def _blend_accumulate(acc: torch.Tensor, y: torch.Tensor, window: tuple[int, int], src_offset: tuple[int, int],
                      acc_offset: tuple[int, int], ramps: tuple[int, int, int, int]) -> None:  # fmt: skip
    """``acc[window at acc_offset] (+)= wy * wx * y[window at src_offset]``: pixels in the top or the left ramp have had an earlier
    contributor (tiles arrive in row-major order) and are added to; every other pixel is stored, so ``acc`` needs no zero fill.
    GPU tensors: one launch of ``rsa_tile_blend_accumulate``; CPU tensors (the oracle-driven tests): the same formula in torch."""
    if acc.is_cuda:
        from .engine import ops

        return ops.tile_blend_accumulate(acc, y, window, src_offset, acc_offset, ramps)
    (wh, ww), (sy, sx), (py, px), (top, bottom, left, right) = window, src_offset, acc_offset, ramps
    if _is_image(y):
        src = y[:, sy : sy + wh, sx : sx + ww].permute(0, 3, 1, 2).to(torch.float32) / 255
    else:
        src = y[:, :, sy : sy + wh, sx : sx + ww].to(torch.float32)
    v = src * (_ramp(wh, top, bottom, y.device)[:, None] * _ramp(ww, left, right, y.device)[None, :])
    dst = acc[:, :, py : py + wh, px : px + ww]
    dst[:, :, top:, left:] = v[:, :, top:, left:]
    dst[:, :, :top] += v[:, :, :top]
    dst[:, :, top:, :left] += v[:, :, top:, :left]


def _blend_tiles(model, x: torch.Tensor, scale: int, tiles: Sequence[Tile], blend: int) -> tuple[torch.Tensor, torch.dtype]:
    """The blended f32 ``[N, C, H*scale, W*scale]`` frame of ``tiles`` (in ``Tile.index`` order, which the store / accumulate rule needs)
    and the dtype of the model's outputs."""
    img = _is_image(x)
    n = x.shape[0]
    h, w = (x.shape[1], x.shape[2]) if img else (x.shape[2], x.shape[3])
    acc = None
    for t in sorted(tiles, key=lambda t: t.index):
        crop = (x[:, t.ry0 : t.ry1, t.rx0 : t.rx1] if img else x[:, :, t.ry0 : t.ry1, t.rx0 : t.rx1]).contiguous()
        y = model(crop)
        if acc is None:
            acc = torch.empty((n, y.shape[3] if img else y.shape[1], h * scale, w * scale), dtype=torch.float32, device=y.device)
        py0, py1, px0, px1, *ramps = blend_window(t, h, w, blend, scale)
        _blend_accumulate(acc, y, (py1 - py0, px1 - px0), (py0 - t.ry0 * scale, px0 - t.rx0 * scale), (py0, px0), tuple(ramps))
    return acc, y.dtype


def _image_from_acc(acc: torch.Tensor) -> torch.Tensor:
    """f32 ``[N, C, H, W]`` -> uint8 ``[N, H, W, C]``: clamp to [0, 1], times 255, round half to even."""
    if acc.is_cuda:
        from .engine import ops

        return ops.nchw_to_image_u8(acc)
    return (acc.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


RESAMPLE_FILTERS = ('bicubic', 'bilinear')
RESAMPLE_MAX_RATIO = 8  # source pixels per output pixel along an axis: bounds the taps (33 for bicubic) and the band a workgroup stages


def _bicubic(t: float) -> float:
    """Keys' cubic with a = -0.5."""
    t = abs(t)
    if t < 1.0:
        return ((-0.5 + 2.0) * t - (-0.5 + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * -0.5
    return 0.0


def _triangle(t: float) -> float:
    t = abs(t)
    return 1.0 - t if t < 1.0 else 0.0


@functools.lru_cache(maxsize=64)
def resample_table(n_in: int, n_out: int, filter: str = 'bicubic', dtype: torch.dtype = torch.float32) -> tuple[torch.Tensor, torch.Tensor]:
    """The weights with which an axis of ``n_in`` pixels is resampled to ``n_out``: ``(start int32 [n_out], weight float32 [n_out, taps])``,
    output ``i`` = sum over ``j`` of ``weight[i, j] * source[start[i] + j]``.  A restatement of what torch's CPU
    ``F.interpolate(mode=filter, antialias=True, align_corners=False)`` computes, made in f64 and rounded to f32 once.
    Rows shorter than ``taps`` are padded with zero weights; ``start + taps <= n_in`` holds for every row (a row that would leave the
    axis is shifted down, its zeros in front).  ``dtype = torch.float64`` returns the weights before that rounding (for checks against
    torch).  The tensors are shared between callers: do not write to them."""
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f'resample filter {filter!r} is not one of {RESAMPLE_FILTERS}')
    if n_in < 1 or n_out < 1:
        raise ValueError(f'cannot resample {n_in} pixels to {n_out}: both sizes must be >= 1')
    if n_in > RESAMPLE_MAX_RATIO * n_out:
        raise ValueError(f'resampling {n_in} pixels to {n_out} shrinks by more than {RESAMPLE_MAX_RATIO}')
    f, size = (_bicubic, 4) if filter == 'bicubic' else (_triangle, 2)
    scale = n_in / n_out
    support = size / 2 * scale if scale >= 1.0 else size / 2
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    rows = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        w = [f((j + lo - c + 0.5) * inv) for j in range(hi - lo)]
        total = sum(w)
        rows.append((lo, [v / total for v in w]))
    taps = max(len(w) for _, w in rows)
    start = torch.empty(n_out, dtype=torch.int32)
    weight = torch.zeros((n_out, taps), dtype=torch.float64)
    for i, (lo, w) in enumerate(rows):
        s = min(lo, n_in - taps)
        start[i] = s
        weight[i, lo - s : lo - s + len(w)] = torch.tensor(w, dtype=torch.float64)
    return start, weight.to(dtype)


_RESAMPLE_DEVICE_TABLES: dict = {}


def resample_tables_device(n_in: int, n_out: int, filter: str, device) -> tuple[torch.Tensor, torch.Tensor]:
    """``resample_table`` on ``device``, copied there once per ``(n_in, n_out, filter, device)``."""
    key = (n_in, n_out, filter, str(device))
    hit = _RESAMPLE_DEVICE_TABLES.get(key)
    if hit is None:
        if len(_RESAMPLE_DEVICE_TABLES) >= 64:
            _RESAMPLE_DEVICE_TABLES.clear()
        start, weight = resample_table(n_in, n_out, filter)
        hit = _RESAMPLE_DEVICE_TABLES[key] = (start.to(device), weight.to(device))
    return hit


def _check_out_args(out_size, out_scale, resample: str) -> None:
    """The refusals of ``out_size`` / ``out_scale`` / ``resample`` that need neither the image nor the model."""
    if out_size is not None and out_scale is not None:
        raise ValueError('give out_size or out_scale, not both')
    if resample not in RESAMPLE_FILTERS:
        raise ValueError(f'resample = {resample!r} is not one of {RESAMPLE_FILTERS}')
    if out_scale is not None and not out_scale > 0:
        raise ValueError(f'out_scale = {out_scale} must be positive')
    if out_size is not None and (len(out_size) != 2 or any(int(v) != v or v < 1 for v in out_size)):
        raise ValueError(f'out_size = {out_size} must be (rows, columns), both >= 1')


def _target_size(h: int, w: int, scale: int, out_size, out_scale, resample: str) -> tuple[int, int] | None:
    """The size to deliver an ``h`` x ``w`` input at, or None when that is the model's native ``h * scale`` x ``w * scale`` (nothing to
    do).  ``out_scale`` counts from the INPUT size.  Raises before the model runs when an axis would shrink by more than 8."""
    _check_out_args(out_size, out_scale, resample)
    if out_size is None and out_scale is None:
        return None
    if out_scale is not None:
        target = max(1, math.floor(h * out_scale + 0.5)), max(1, math.floor(w * out_scale + 0.5))
    else:
        target = int(out_size[0]), int(out_size[1])
    native = h * scale, w * scale
    if target == native:
        return None
    for n_in, n_out in zip(native, target):
        if n_in > RESAMPLE_MAX_RATIO * n_out:
            raise ValueError(f'out size {target} shrinks the native {native} frame by more than {RESAMPLE_MAX_RATIO} ({n_in} -> {n_out})')
    return target


def _resample_axis(v: torch.Tensor, table: tuple[torch.Tensor, torch.Tensor], dim: int) -> torch.Tensor:
    """f32 ``v`` with axis ``dim`` (2 or 3 of ``[N, C, H, W]``) filtered by ``table``: taps in ascending order from zero, as the kernel."""
    start, weight = table
    start = start.to(torch.int64)
    shape = (-1, 1) if dim == 2 else (-1,)
    acc = torch.zeros(v.shape[:dim] + (start.numel(),) + v.shape[dim + 1 :], dtype=torch.float32)
    for t in range(weight.shape[1]):
        acc = torch.addcmul(acc, weight[:, t].reshape(shape), v.index_select(dim, start + t))
    return acc


def _resample_frame(y: torch.Tensor, size: tuple[int, int], filter: str, dtype: torch.dtype) -> torch.Tensor:
    """The native frame ``y`` (float ``[N, C, H, W]`` or a uint8 ``[N, H, W, C]`` image) at ``size`` as ``dtype``: uint8 means an
    ``[N, rows, columns, C]`` image (clamp, times 255, round half to even, once), a float dtype an ``[N, C, rows, columns]`` tensor.
    GPU tensors: one launch of ``rsa_resample``; CPU tensors (the oracle-driven tests): the same tables in torch, rows after columns."""
    if y.is_cuda:
        from .engine import ops

        return ops.resample_to_image_u8(y, size, filter) if dtype == torch.uint8 else ops.resample(y, size, filter, dtype)
    v = y.permute(0, 3, 1, 2).to(torch.float32) / 255 if _is_image(y) else y.to(torch.float32)
    v = _resample_axis(v, resample_table(v.shape[3], size[1], filter), 3)
    v = _resample_axis(v, resample_table(v.shape[2], size[0], filter), 2)
    if dtype == torch.uint8:
        return (v.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return v.to(dtype)


def upscale_tiled(model, x: torch.Tensor, scale: int, tile: tuple[int, int], halo: int = 32, align: int = 1, check: bool = True,
                  blend: int = 0, blend_dtype: torch.dtype | None = None, out_size: tuple[int, int] | None = None,
                  out_scale: float | None = None, resample: str = 'bicubic') -> torch.Tensor:  # fmt: skip
    """Single-device tiling of a large image: bounds the engine's activation buffers (e.g. 8K inputs).  ``x``: a float ``[N, C, H, W]``
    tensor, or a uint8 ``[N, H, W, C]`` image for models with ``supports_u8`` (the layouts ``run_tile`` / ``TileParallel`` take).

    ``blend`` (input pixels, default 0 = crop every halo and paste the tiles side by side): cross-fade neighbouring tiles over a band of
    ``2 * blend`` input pixels centred on every interior tile edge, with weights that sum to one (``blend_window``).  It hides the step at
    which two tiles meet when the halo does not cover the model's whole reach (``global_statistics`` models, MoESR); the result still
    differs from the untiled one.  The band is cut out of the halo that is computed anyway, so ``blend <= halo`` (after ``align`` rounded
    the halo up), and the context behind the outer edge of a band is ``halo - blend`` pixels.  ``2 * blend`` may not exceed a tile's extent
    along an axis with several tiles.  The tiles are summed in f32 and the sum is cast to the model's output dtype (``blend_dtype``
    names another one: ``upscale`` keeps the f32 sum for its 8-bit conversion), or rounded to 8 bits for images.  An image that fits one
    tile ignores ``blend``.

    ``out_size = (rows, columns)`` or ``out_scale`` (a positive factor of the INPUT size, each axis rounded half up, at least 1): deliver
    the frame at that size instead of ``H * scale`` x ``W * scale``.  The assembled native frame (the pasted tiles, or the f32 sum of a
    blend) is resampled once with torch's antialiased ``resample`` filter ('bicubic' or 'bilinear': ``resample_table``), by one launch
    of ``rsa_resample`` that also casts to the model's dtype (``blend_dtype`` as above) or rounds to 8 bits.  An axis may shrink by at
    most 8 and grow without limit; the native size, or neither argument, changes nothing."""
    if x.dim() != 4:
        raise ValueError(f'expected a [N, C, H, W] tensor or a uint8 [N, H, W, C] image, got shape {tuple(x.shape)}')
    if blend < 0:
        raise ValueError(f'blend = {blend} must be >= 0')
    img = _is_image(x)
    n = x.shape[0]
    h, w = (x.shape[1], x.shape[2]) if img else (x.shape[2], x.shape[3])
    target = _target_size(h, w, scale, out_size, out_scale, resample)
    rows, cols = -(-h // tile[0]), -(-w // tile[1])
    warn_global_statistics(model, rows * cols)
    tiles = plan_tiles(h, w, rows, cols, halo, align)
    if blend > 0 and len(tiles) > 1:
        _check_blend(tiles, blend, halo, align)
        acc, dtype = _blend_tiles(model, x, scale, tiles, blend)
        if target is not None:
            out = _resample_frame(acc, target, resample, torch.uint8 if img else (dtype if blend_dtype is None else blend_dtype))
        else:
            out = _image_from_acc(acc) if img else acc.to(dtype if blend_dtype is None else blend_dtype)
        return _finish(out) if check else out
    out = None
    for t in tiles:
        y = run_tile(model, x, t, scale)
        if out is None:
            shape = (n, h * scale, w * scale, y.shape[3]) if img else (n, y.shape[1], h * scale, w * scale)
            out = torch.empty(shape, dtype=y.dtype, device=y.device)
        if img:
            out[:, t.y0 * scale : t.y1 * scale, t.x0 * scale : t.x1 * scale] = y
        else:
            out[:, :, t.y0 * scale : t.y1 * scale, t.x0 * scale : t.x1 * scale] = y
    if target is not None:
        out = _resample_frame(out, target, resample, out.dtype)
    return _finish(out) if check else out


def upscale(model, image: torch.Tensor, tile: tuple[int, int] | None = None, halo: int = 32, align: int = 1,
            dtype: torch.dtype = torch.float16, scale: int | None = None, blend: int = 0, out_size: tuple[int, int] | None = None,
            out_scale: float | None = None, resample: str = 'bicubic') -> torch.Tensor:
    """uint8 image in, uint8 image out: ``image`` is [H, W, C] or [N, H, W, C] uint8 on the GPU (what an image decoder delivers).

    ``/255`` and the NHWC->NCHW transpose run in one kernel, the model runs on ``dtype`` tensors (whole image, or ``tile``-sized tiles
    with ``halo`` pixels of context when the image is larger than ``tile``), and ``clamp(0, 1) * 255`` + round-half-even + NCHW->NHWC
    run in one kernel.  The reference leaves both conversions and the tiling to its callers.
    ``align``: SwinIR-family models want tile origins on a window multiple.
    ``blend`` (input pixels, at most ``halo``; 0 = hard crop): cross-fade neighbouring tiles over ``2 * blend`` input pixels around every
    interior tile edge instead of letting them meet at a step (``upscale_tiled``); the context behind the outer edge of a band is
    ``halo - blend`` pixels.  The tiles are summed in f32 and rounded to 8 bits once.  An image that fits one tile ignores it.
    ``out_size = (rows, columns)`` or ``out_scale`` (a positive factor of the INPUT size: a x4 model at ``out_scale = 2`` delivers x2; each
    axis rounded half up, at least 1): deliver the image at that size.  The native frame -- the model's output, the pasted tiles, or the f32
    sum of a blend -- is read once by one launch of ``rsa_resample``, which applies torch's antialiased ``resample`` filter ('bicubic' or
    'bilinear') and the 8-bit conversion together: it takes the place of the conversion kernel and the image is rounded once, after the
    filter.  An axis may shrink by at most 8 and grow without limit.  The native size, or neither argument: nothing changes.
    """
    from .engine import ops

    if blend < 0:
        raise ValueError(f'blend = {blend} must be >= 0')
    _check_out_args(out_size, out_scale, resample)
    if getattr(model, 'supports_u8', False) and image.dtype == torch.uint8:
        return _upscale_u8(model, image, tile, halo, align, scale, blend, out_size, out_scale, resample)
    squeeze = image.dim() == 3
    x = ops.image_u8_to_nchw(image, dtype)
    if scale is None:
        scale = model.parameters_info.upscale
        if not isinstance(scale, int):
            raise ValueError('this model has several output scales: pass scale=')
    _, _, h, w = x.shape
    target = _target_size(h, w, scale, out_size, out_scale, resample)
    if tile is None or (h <= tile[0] and w <= tile[1]):
        y = model(x)
    else:
        y = upscale_tiled(model, x, scale, tile, halo, align, check=False, blend=blend, blend_dtype=torch.float32)
    out = _finish(ops.nchw_to_image_u8(y) if target is None else ops.resample_to_image_u8(y, target, resample))
    return out[0] if squeeze else out


def upscale_yuv(model, y: torch.Tensor, uv: torch.Tensor, fmt: str = 'nv12', out_fmt: str | None = None, matrix: str = 'bt709',
                range: str = 'limited', chroma_loc: str = 'left', tile: tuple[int, int] | None = None, halo: int = 32, align: int = 1,
                blend: int = 0, dtype: torch.dtype = torch.float16, scale: int | None = None, out_size: tuple[int, int] | None = None,
                out_scale: float | None = None, resample: str = 'bicubic') -> tuple[torch.Tensor, torch.Tensor]:
    """Video frame in, video frame out: two-plane Y'CbCr 4:2:0 as a GPU video decoder delivers it and an encoder accepts it.

    ``y`` is ``[H, W]`` or ``[N, H, W]``, ``uv`` ``[H/2, W/2, 2]`` or ``[N, H/2, W/2, 2]`` interleaved (Cb, Cr): ``torch.uint8`` for
    ``fmt = 'nv12'``, ``torch.uint16`` words with the code in their top 10 bits for ``'p010'``; a pitched surface is passed as a
    row-strided view.  Returns the contiguous planes ``(y, uv)`` of the upscaled frame in ``out_fmt`` (default: ``fmt``;
    ``out_fmt='p010'`` with NV12 input delivers an 8-bit source in 10 bits).  ``matrix`` ('bt601' / 'bt709' / 'bt2020'), ``range``
    ('limited' / 'full') and ``chroma_loc`` ('left': the H.264 / HEVC default; 'center') describe the input and the output alike
    (``ops.yuv420_to_nchw`` has the definition); the transfer function is untouched.

    One kernel turns the planes into the ``dtype`` R'G'B' tensor the model reads (chroma interpolated linearly), the model runs on the
    whole frame or on ``tile``-sized tiles exactly as in ``upscale`` (``halo``, ``align``, ``blend``: see there; models with
    ``supports_u8`` take this float path too), ``out_size`` / ``out_scale`` / ``resample`` resample the native frame once to f32 (rules
    and errors of ``upscale``; the delivered size must be even), and one kernel writes both planes: the frame is rounded to codes
    once, at the end.  float16 carries 11 bits: with ``out_fmt='p010'``, ``dtype=torch.float32`` keeps the tenth bit clean."""
    from .engine import ops

    if out_fmt is None:
        out_fmt = fmt
    ops._yuv_args(fmt, matrix, range, chroma_loc)
    ops._yuv_args(out_fmt, matrix, range, chroma_loc)
    if blend < 0:
        raise ValueError(f'blend = {blend} must be >= 0')
    _check_out_args(out_size, out_scale, resample)
    info = getattr(model, 'parameters_info', None)
    if info is not None and (info.in_channels != 3 or info.out_channels != 3):
        raise ValueError(f'upscale_yuv needs a model with 3 channels in and out, got {info.in_channels} in and {info.out_channels} out')
    if scale is None:
        scale = getattr(info, 'upscale', None)
        if not isinstance(scale, int):
            raise ValueError('this model does not name one output scale: pass scale=')
    squeeze = y.dim() == 2
    y, uv = ops._yuv_planes(y, uv, fmt)  # ValueError for shapes or dtypes that disagree with fmt, and for odd sizes
    _, h, w = y.shape
    target = _target_size(h, w, scale, out_size, out_scale, resample)
    if target is not None and (target[0] % 2 or target[1] % 2):
        raise ValueError(f'a 4:2:0 frame has an even size: the output size {target} is odd')
    x = ops.yuv420_to_nchw(y, uv, fmt, matrix, range, chroma_loc, dtype)
    if tile is None or (h <= tile[0] and w <= tile[1]):
        out = model(x)
    else:
        out = upscale_tiled(model, x, scale, tile, halo, align, check=False, blend=blend, blend_dtype=torch.float32)
    if target is not None:
        out = _resample_frame(out, target, resample, torch.float32)
    oy, ouv = ops.nchw_to_yuv420(out, out_fmt, matrix, range, chroma_loc)
    _finish(oy)
    return (oy[0], ouv[0]) if squeeze else (oy, ouv)


def upscale_rgba(model, image: torch.Tensor, alpha: str = 'model', bleed: int = 8, out_bits: int | None = None,
                 tile: tuple[int, int] | None = None, halo: int = 32, align: int = 1, blend: int = 0, dtype: torch.dtype = torch.float16,
                 scale: int | None = None, out_size: tuple[int, int] | None = None, out_scale: float | None = None,
                 resample: str = 'bicubic') -> torch.Tensor:
    """Still image in, still image out, with alpha, gray and 16 bits: ``image`` is ``[H, W, C]`` or ``[N, H, W, C]``, ``torch.uint8`` or
    ``torch.uint16`` (codes over the full range 0 .. 65535), ``C`` = 1 gray, 2 gray + alpha, 3 RGB, 4 RGBA; alpha is straight, not
    premultiplied.  A row-strided view whose innermost two strides are dense is read in place.  Returns the contiguous image of the same
    rank and ``C`` at the size ``upscale`` would deliver, in ``out_bits`` = 8 or 16 (default: the input's depth; 16 bits from an 8-bit
    source is how a gradient avoids banding).

    The model has ``in_channels == out_channels`` of 1 or 3.  A three-channel model reads a gray image in all three channels and the
    delivered gray is the mean of its three output channels; a one-channel model takes gray images only.  Models with ``supports_u8``
    take this float path too.

    ``alpha='model'``: alpha, replicated to the model's channels, goes through the model as ``N`` further batch entries of the same call
    (one call per tile on a batch of ``2 N``), and the delivered alpha is the mean of the output channels.  ``alpha='resample'``: alpha is
    resampled to the delivered size with the ``resample`` filter in f32 (``rsa_resample``); the model sees colour only.  When no alpha
    code of the batch is below the maximum both modes skip the alpha work and deliver the maximum code: an opaque RGBA image costs what
    the RGB image costs.  The colour stored under fully transparent pixels (usually black) would bleed a dark fringe into the visible
    edge through the model's receptive field, so the input kernel replaces it by colour bled in from the visible pixels over ``bleed``
    (0 .. 16) pixels (``ops.image_to_nchw_alpha`` / csrc/rgba.hip have the definition); alpha and the colour of every pixel with
    ``alpha > 0`` are never changed.  Images without an alpha channel ignore ``alpha`` and ``bleed``.

    ``tile``, ``halo``, ``align``, ``blend``, ``scale``, ``out_size``, ``out_scale`` and ``resample`` keep the rules and the errors of
    ``upscale``.  Blend sums and resampling stay in f32 and the image is rounded to codes once, at the end.  float16 carries 11 bits:
    with ``out_bits=16``, ``dtype=torch.float32`` keeps the low bits of the result clean.  For a uint8 RGB image, ``out_bits=8`` and a
    model without ``supports_u8`` the result equals ``upscale``'s."""
    from .engine import ops

    if alpha not in ('model', 'resample'):
        raise ValueError(f"alpha = {alpha!r} is not one of ('model', 'resample')")
    bleed = ops._check_bleed(bleed)
    if blend < 0:
        raise ValueError(f'blend = {blend} must be >= 0')
    _check_out_args(out_size, out_scale, resample)
    squeeze = image.dim() == 3
    img, bits = ops._image_args(image, 'upscale_rgba')
    if out_bits is None:
        out_bits = bits
    if out_bits not in (8, 16):
        raise ValueError(f'out_bits = {out_bits} must be 8 or 16')
    n, h, w, c = img.shape
    info = getattr(model, 'parameters_info', None)
    cm = 3
    if info is not None:
        if info.in_channels != info.out_channels or info.in_channels not in (1, 3):
            raise ValueError(f'upscale_rgba needs a model with 1 or 3 channels in and as many out, got {info.in_channels} in and {info.out_channels} out')
        cm = info.in_channels
    if c >= 3 and cm == 1:
        raise ValueError(f'a one-channel model takes gray images only, got an image of {c} channels')
    if scale is None:
        scale = getattr(info, 'upscale', None)
        if not isinstance(scale, int):
            raise ValueError('this model does not name one output scale: pass scale=')
    target = _target_size(h, w, scale, out_size, out_scale, resample)
    x, a, flags = ops.image_to_nchw_alpha(img, cm, alpha, bleed, dtype)
    translucent = flags is not None and bool(flags.any())  # the one host read of the call: it decides the batch the model sees
    if not translucent:
        x, a = x[:n], None
    if tile is None or (h <= tile[0] and w <= tile[1]):
        out = model(x)
    else:
        out = upscale_tiled(model, x, scale, tile, halo, align, check=False, blend=blend, blend_dtype=torch.float32)
    if target is not None:
        out = _resample_frame(out, target, resample, torch.float32)
    src = None
    if translucent and alpha == 'model':
        out, src = out[:n], out[n:]
    elif translucent:
        size = tuple(out.shape[2:])
        src = a if size == (h, w) else _resample_frame(a, size, resample, torch.float32)
    out = _finish(ops.nchw_to_image_alpha(out, src, c, out_bits))
    return out[0] if squeeze else out


def _upscale_u8(model, image: torch.Tensor, tile, halo: int, align: int, scale, blend: int = 0, out_size=None, out_scale=None,
                resample: str = 'bicubic') -> torch.Tensor:  # fmt: skip
    """``upscale`` for models that read and write 8-bit images themselves (no separate conversion passes): whole image, or tiles
    (``blend > 0``: the tiles' 8-bit codes are cross-faded in f32 and rounded once, see ``upscale_tiled``).  Another output size: the
    model's 8-bit image, the pasted 8-bit tiles or the f32 sum of the blend is resampled and rounded by one launch."""
    squeeze = image.dim() == 3
    img = image.unsqueeze(0) if squeeze else image
    if scale is None:
        scale = model.parameters_info.upscale
    n, h, w, c = img.shape
    if tile is None or (h <= tile[0] and w <= tile[1]):
        target = _target_size(h, w, scale, out_size, out_scale, resample)
        out = model(img)
        if target is not None:
            out = _resample_frame(out, target, resample, torch.uint8)
    else:
        out = upscale_tiled(model, img, scale, tile, halo, align, check=False, blend=blend, out_size=out_size, out_scale=out_scale, resample=resample)
    out = _finish(out)
    return out[0] if squeeze else out


class TileParallel:
    """``TileParallel(model, scale)(x)``: every rank of the process group upscales its share of the tiles of ``x`` and
    all ranks return the complete upscaled image.

    ``x`` must be the same full input on every rank (a 3-channel image is cheap to replicate; only the outputs and
    the activations are large): a float ``[N, C, H, W]`` tensor, or -- for models with ``supports_u8`` -- a uint8
    ``[N, H, W, C]`` image, in which case the tiles that cross the links are 8-bit (a quarter of the fp32 bytes).
    With ``world_size`` ranks the image is cut into ``world_size`` tiles (one per rank) unless ``grid`` says otherwise;
    tiles are dealt round-robin: rank r owns tiles r, r + world, ...

    The collective: one ``all_gather_into_tensor`` per ROUND of tiles (round k = tiles k*world .. k*world + world - 1),
    issued asynchronously as soon as this rank's tile of the round is finished, so it runs (on the backend's own stream)
    beside the computation of the next round's tile; all of them are waited for once, at the end.  When the tiles of a
    round are equal full-width row bands of a channel-interleaved image (uint8 ``[1, H, W, C]``: the bands of a round are
    one contiguous slab of the result) the gather writes straight into the result; otherwise tiles are padded to the
    largest tile, gathered into a receive buffer and copied into place.

    The result has the model's native size; a caller who wants another one resamples the gathered result with ``ops.resample`` /
    ``ops.resample_to_image_u8`` (what ``upscale(out_size=)`` does on one device).
    """

    def __init__(self, model: Callable[[torch.Tensor], torch.Tensor], scale: int, halo: int = 32, align: int = 1,
                 grid: tuple[int, int] | None = None, group=None, overlap: bool = True):  # fmt: skip
        self.model, self.scale, self.halo, self.align, self.grid, self.group, self.overlap = model, scale, halo, align, grid, group, overlap
        self.last_stats: dict = {}

    def tiles_for(self, height: int, width: int, world: int) -> list[Tile]:
        rows, cols = self.grid if self.grid is not None else choose_grid(world, height, width)
        return plan_tiles(height, width, rows, cols, self.halo, self.align)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            world, rank = 1, 0
        else:
            world, rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        img = _is_image(x)
        n = x.shape[0]
        h, w = (x.shape[1], x.shape[2]) if img else (x.shape[2], x.shape[3])
        s = self.scale
        tiles = self.tiles_for(h, w, world)
        warn_global_statistics(self.model, len(tiles))
        mine = tiles[rank::world]

        def full_shape(c_out):
            return (n, h * s, w * s, c_out) if img else (n, c_out, h * s, w * s)

        def place(full, t, o):
            if img:
                full[:, t.y0 * s : t.y1 * s, t.x0 * s : t.x1 * s] = o
            else:
                full[:, :, t.y0 * s : t.y1 * s, t.x0 * s : t.x1 * s] = o

        if world == 1:
            full = None
            for t in mine:
                o = run_tile(self.model, x, t, s)
                if full is None:
                    full = torch.empty(full_shape(o.shape[3] if img else o.shape[1]), dtype=o.dtype, device=o.device)
                place(full, t, o)
            return _finish(full)

        rounds = -(-len(tiles) // world)
        # Can the gather of a round land in the result itself?  Channel-interleaved single image, every tile a full-width row band,
        # every round complete and made of equal bands.
        in_place = img and n == 1 and len(tiles) == rounds * world and all(t.x0 == 0 and t.x1 == w for t in tiles) and all(
            len({t.shape[0] for t in tiles[k * world : (k + 1) * world]}) == 1 for k in range(rounds))  # fmt: skip
        mh = max(t.shape[0] for t in tiles) * s
        mw = max(t.shape[1] for t in tiles) * s
        full = recv = None
        works, keep = [], []
        c_out = dtype = device = None
        for k in range(rounds):
            t = mine[k] if k < len(mine) else None
            o = run_tile(self.model, x, t, s) if t is not None else None
            if c_out is None:
                ref = o if (o is not None and o.numel()) else None
                c_out, dtype, device = self._out_meta(ref, x, img, idle_ranks=len(tiles) < world)
                full = torch.empty(full_shape(c_out), dtype=dtype, device=device)
                if not in_place:
                    recv = torch.empty((rounds, world, n, mh, mw, c_out) if img else (rounds, world, n, c_out, mh, mw), dtype=dtype, device=device)
            if in_place:
                band = tiles[k * world]
                dst = full[0, band.y0 * s : tiles[k * world + world - 1].y1 * s].reshape(-1)  # the round's bands: one contiguous slab
                src = o.reshape(-1) if o.is_contiguous() else o.contiguous().reshape(-1)
                out_t, in_t = dst, src
            else:
                send = torch.zeros((n, mh, mw, c_out) if img else (n, c_out, mh, mw), dtype=dtype, device=device)
                if o is not None and o.numel():
                    if img:
                        send[:, : o.shape[1], : o.shape[2]] = o
                    else:
                        send[:, :, : o.shape[2], : o.shape[3]] = o
                out_t, in_t = recv[k].reshape(-1), send.reshape(-1)
            keep.append(in_t)  # the input of an asynchronous collective must stay untouched (and alive) until it is waited for
            work = dist.all_gather_into_tensor(out_t, in_t, group=self.group, async_op=self.overlap)
            if self.overlap:
                works.append(work)
        for wk in works:
            wk.wait()
        if not in_place:
            for t in tiles:
                k, r = t.index // world, t.index % world
                th, tw = t.shape
                place(full, t, recv[k, r, :, : th * s, : tw * s] if img else recv[k, r, :, :, : th * s, : tw * s])
        self.last_stats = dict(rounds=rounds, in_place=bool(in_place), bytes_per_round=int(keep[0].numel() * keep[0].element_size()) * world,
                               tile_dtype=str(dtype), overlap=bool(self.overlap))  # fmt: skip
        return _finish(full)

    def _out_meta(self, ref, x, img: bool, idle_ranks: bool):
        """(channels, dtype, device) of the output tiles.  Only when there are fewer tiles than ranks can a rank have no
        output of its own; ``idle_ranks`` is the same on every rank, so all of them enter the exchange together."""
        import torch.distributed as dist

        if not idle_ranks:
            return (ref.shape[3] if img else ref.shape[1]), ref.dtype, ref.device
        mine = None if ref is None else ((ref.shape[3] if img else ref.shape[1]), ref.dtype)
        metas = [None] * dist.get_world_size(self.group)
        dist.all_gather_object(metas, mine, group=self.group)
        c_out, dtype = next(m for m in metas if m is not None)
        return c_out, dtype, (ref.device if ref is not None else x.device)
