"""f64 references of ``upscale(out_size=)`` that import nothing of the code under test.

``interpolate64`` is torch's CPU ``F.interpolate(mode, antialias=True, align_corners=False)`` on float64 tensors: the definition.
``apply_tables`` applies an axis table ``(start, weight)`` -- output ``i`` = sum over ``j`` of ``weight[i, j] * source[start[i] + j]`` -- in
f64; tests/test_resample.py pins it (with the tables of the code under test) to ``interpolate64`` within 1e-12.
``bound`` is the error an f32 evaluation of two such tables may show against the f64 value:
``B = (T_h + T_w + 4) * 2^-24 * S_h * S_w * max(1, |x|max)`` with ``T`` = taps and ``S`` = the largest row sum of |weights| of each table
(two fmaf chains of ``T`` terms, plus one rounding of each weight)."""

import torch
import torch.nn.functional as F


def interpolate64(x: torch.Tensor, size, mode: str) -> torch.Tensor:
    """``x``: ``[N, C, h, w]`` (any float dtype, taken to f64) -> f64 ``[N, C, rows, columns]``."""
    return F.interpolate(x.to(torch.float64), size=tuple(size), mode=mode, antialias=True, align_corners=False)


def apply_axis(x: torch.Tensor, table, dim: int) -> torch.Tensor:
    """f64 ``x`` with axis ``dim`` replaced by the table's outputs."""
    start, weight = table
    start, weight = start.to(torch.int64), weight.to(torch.float64)
    idx = start[:, None] + torch.arange(weight.shape[1])[None, :]  # [n_out, taps]
    assert int(idx.min()) >= 0 and int(idx.max()) < x.shape[dim], 'a table row leaves the axis'
    g = x.index_select(dim, idx.reshape(-1))
    g = g.reshape(x.shape[:dim] + idx.shape + x.shape[dim + 1 :])  # [..., n_out, taps, ...]
    shape = [1] * g.dim()
    shape[dim], shape[dim + 1] = weight.shape
    return (g * weight.reshape(shape)).sum(dim + 1)


def apply_tables(x: torch.Tensor, table_y, table_x) -> torch.Tensor:
    """f64 ``[N, C, rows, columns]`` of ``x`` ``[N, C, h, w]``: columns first, then rows (the order does not matter in f64 beyond 1e-15)."""
    return apply_axis(apply_axis(x.to(torch.float64), table_x, 3), table_y, 2)


def abs_row_sum(table) -> float:
    return table[1].to(torch.float64).abs().sum(1).max().item()


def bound(table_y, table_x, xmax: float) -> float:
    return (table_y[1].shape[1] + table_x[1].shape[1] + 4) * 2.0**-24 * abs_row_sum(table_y) * abs_row_sum(table_x) * max(1.0, xmax)


def image_as_f64(img: torch.Tensor) -> torch.Tensor:
    """uint8 ``[N, H, W, C]`` codes -> f64 ``[N, C, H, W]`` in [0, 1]."""
    return img.permute(0, 3, 1, 2).to(torch.float64) / 255


def image_error(got: torch.Tensor, want01: torch.Tensor) -> float:
    """Largest distance, in codes, of the uint8 ``[N, H, W, C]`` image ``got`` from ``255 * clamp(want01, 0, 1)`` (f64 ``[N, C, H, W]``)."""
    return (got.permute(0, 3, 1, 2).to(torch.float64) - 255 * want01.clamp(0, 1)).abs().max().item()
