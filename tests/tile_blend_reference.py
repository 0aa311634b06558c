"""f64 restatement of the seam-blending weights of the tiler, written from their definition and importing nothing of the code under test.

Per axis, in output pixels: a tile owns input pixels ``[a0, a1)`` of an axis of length ``size``; ``s`` = scale, ``B = blend * s``.
It contributes ``[a0*s - B, a1*s + B)`` (no ``-B`` at ``a0 = 0``, no ``+B`` at ``a1 = size``).  Where ``a0 > 0``, the pixels ``p`` of
``[a0*s - B, a0*s + B)`` weigh ``u = (p - (a0*s - B) + 0.5) / (2B)``; where ``a1 < size``, those of ``[a1*s - B, a1*s + B)`` weigh
``1 - u`` with ``u`` from the same expression at that seam; every other pixel of the range weighs 1, every pixel outside it 0.
The 2-D weight is ``wy(py) * wx(px)``.

A tile is anything with ``y0, y1, x0, x1`` (owned region) and ``ry0, rx0`` (origin of what the model read), in input pixels.
"""

import torch


def axis_weights(a0: int, a1: int, size: int, blend: int, scale: int) -> torch.Tensor:
    """f64 weights of the tile ``[a0, a1)`` over the WHOLE output axis ``[0, size * scale)`` (0 outside the contribution range)."""
    s, b = scale, blend * scale
    w = torch.zeros(size * s, dtype=torch.float64)
    lo = a0 * s - (b if a0 > 0 else 0)
    hi = a1 * s + (b if a1 < size else 0)
    for p in range(lo, hi):
        v = 1.0
        if a0 > 0 and a0 * s - b <= p < a0 * s + b:
            v = (p - (a0 * s - b) + 0.5) / (2 * b)
        if a1 < size and a1 * s - b <= p < a1 * s + b:
            v = 1.0 - (p - (a1 * s - b) + 0.5) / (2 * b)
        w[p] = v
    return w


def tile_weights(tile, height: int, width: int, blend: int, scale: int) -> torch.Tensor:
    """f64 ``[height * scale, width * scale]`` weight of one tile."""
    return axis_weights(tile.y0, tile.y1, height, blend, scale)[:, None] * axis_weights(tile.x0, tile.x1, width, blend, scale)[None, :]


def band_mask(tiles, height: int, width: int, blend: int, scale: int) -> torch.Tensor:
    """bool ``[height * scale, width * scale]``: the pixels at which some tile weighs strictly between 0 and 1."""
    mask = torch.zeros(height * scale, width * scale, dtype=torch.bool)
    for t in tiles:
        w = tile_weights(t, height, width, blend, scale)
        mask |= (w > 0) & (w < 1)
    return mask


def compose(tiles, outputs, height: int, width: int, blend: int, scale: int) -> torch.Tensor:
    """f64 ``[N, C, height * scale, width * scale]`` blend of the per-tile model outputs ``outputs[i]`` (float ``[N, C, h, w]`` of the read
    window of ``tiles[i]``, origin ``(ry0, rx0)``)."""
    out = None
    for t, y in zip(tiles, outputs):
        y = y.to(torch.float64)
        if out is None:
            out = torch.zeros(y.shape[0], y.shape[1], height * scale, width * scale, dtype=torch.float64)
        w = tile_weights(t, height, width, blend, scale)
        rows, cols = torch.nonzero(w.sum(1)).flatten(), torch.nonzero(w.sum(0)).flatten()
        py0, py1, px0, px1 = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
        sy, sx = py0 - t.ry0 * scale, px0 - t.rx0 * scale
        out[:, :, py0:py1, px0:px1] += w[py0:py1, px0:px1] * y[:, :, sy : sy + py1 - py0, sx : sx + px1 - px0]
    return out


def image_as_f64(img: torch.Tensor) -> torch.Tensor:
    """uint8 ``[N, H, W, C]`` codes -> f64 ``[N, C, H, W]`` in [0, 1]."""
    return img.permute(0, 3, 1, 2).to(torch.float64) / 255


def ramp_weights(length: int, rise: int, fall: int) -> torch.Tensor:
    """f64 weights of one axis of a contributed window given its ramp WIDTHS (what the kernel's entry point takes): rising over the first
    ``rise`` pixels, falling over the last ``fall``.  A window shorter than ``rise + fall`` (which the tiler never plans, but the entry
    point accepts as long as each ramp fits) takes the product of the two ramps where they overlap."""
    w = torch.ones(length, dtype=torch.float64)
    for i in range(length):
        if i < rise:
            w[i] = (i + 0.5) / rise
        if i >= length - fall:
            w[i] = w[i] * (1.0 - (i - (length - fall) + 0.5) / fall)
    return w
