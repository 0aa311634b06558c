#!/usr/bin/env python3
"""What the still-image formats of ``upscale_rgba`` cost at the size a user runs: a 1080 x 1920 RGBA frame in, the 4320 x 7680 frame of
RealESRGAN-x4plus (RRDBNet, 23 blocks) out (profiles/rgba_measure.txt).

  rgba_measure.py kernels [N]
      The launches alone, N of each (default 20) alternated after a warm-up, device events around each (the output allocations included):
      ``rsa_image_to_nchw_alpha`` on a 1080 x 1920 RGBA8 frame to f16 -- opaque with ``bleed`` 0 and 8, and with a transparent region of
      30 % of the frame with ``bleed`` 8 and 16 -- beside the parent's ``rsa_image_u8_to_nchw`` on the RGB frame; ``rsa_nchw_to_image_alpha``
      on the 4320 x 7680 f16 frame to RGBA8 and RGBA16 (alpha from a second f16 tensor, and the constant maximum), beside the parent's
      ``rsa_nchw_to_image_u8``.  Each with its byte model (every operand once) at 8 TB/s.
  rgba_measure.py frames [N]
      N frames (default 8) each of whole calls, alternated in one process after a warm-up, host clock around the call (every call ends in
      a device synchronise): ``upscale_rgba`` on the RGBA frame -- opaque, and with real transparency under ``alpha='model'`` and
      ``alpha='resample'`` -- against ``upscale`` on the RGB image of the same frame, for RRDBNet in 2 x 2 tiles of (540, 960), halo 32,
      and for a Compact network (64 features, 16 convolutions, x4) untiled on f16 tensors; the RGB variant is timed twice (``rgb`` and
      ``rgb again``): their difference is the run-to-run spread.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, SCALE, TILE, HALO = 1080, 1920, 4, (540, 960), 32
WARMUP = 2
BYTES_PER_S = 8e12  # what the project prices a byte at


def _timed(runs, n):
    """``runs``: name -> (callable, byte model).  Alternates them ``n`` times between device events and prints one line each."""
    import torch

    for _ in range(WARMUP):
        for run, _ in runs.values():
            run()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(n):
        for name, (run, _) in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    for name, t in times.items():
        model = runs[name][1]
        med = statistics.median(t)
        print(f'{name}: median {med:.1f} us between device events (min {min(t):.1f}, max {max(t):.1f}, {n} launches, includes the output allocations); '
              f'byte model {model / 1e6:.1f} MB = {model / BYTES_PER_S * 1e6:.1f} us at 8 TB/s: ratio {med * 1e-6 / (model / BYTES_PER_S):.2f}')  # fmt: skip
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def _frame(transparent: bool):
    """The 1080 x 1920 RGBA8 test frame (CPU): random colour; ``transparent``: alpha 0 in an ellipse of 30 % of the frame, a ramp of
    partial alpha 16 pixels wide around it, the maximum elsewhere."""
    import torch

    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (1, H, W, 4), generator=g, dtype=torch.uint8)
    img[..., 3] = 255
    if transparent:
        yy = (torch.arange(H, dtype=torch.float32) - H / 2)[:, None] / (H / 2)
        xx = (torch.arange(W, dtype=torch.float32) - W / 2)[None, :] / (W / 2)
        r = (yy * yy + xx * xx).sqrt() / (0.3 * 4 / 3.14159265) ** 0.5  # r < 1: an ellipse of 30 % of the frame
        img[0, :, :, 3] = ((r - 1) * (H / 2) / 16).clamp(0, 1).mul(255).round().to(torch.uint8)
    return img


def kernels(n):
    import torch

    from resselt_amd.engine import ops

    dev = torch.device('cuda:0')
    px = H * W
    opaque, holed = _frame(False).to(dev), _frame(True).to(dev)
    print(f'transparent frame: {float((holed[..., 3] == 0).float().mean()) * 100:.1f} % of the pixels have alpha 0')
    rgb = opaque[..., :3].contiguous()
    read_bytes = px * (4 + 2 * 3 * 2)  # RGBA8 in, colour and replicated alpha in f16 out
    runs = {'image_u8_to_nchw RGB8 -> f16 1080 x 1920 (parent)': (lambda: ops.image_u8_to_nchw(rgb, torch.float16), px * (3 + 3 * 2))}
    for name, img, bleed in (('opaque, bleed 0', opaque, 0), ('opaque, bleed 8', opaque, 8), ('30 % transparent, bleed 8', holed, 8), ('30 % transparent, bleed 16', holed, 16)):
        runs[f'image_to_nchw_alpha RGBA8 -> f16 {name}'] = (lambda i=img, b=bleed: ops.image_to_nchw_alpha(i, 3, 'model', b, torch.float16), read_bytes)
    med = _timed(runs, n)
    base = med['image_u8_to_nchw RGB8 -> f16 1080 x 1920 (parent)'][0]
    for name, (t, lo, hi) in med.items():
        if name.startswith('image_to_nchw_alpha'):
            print(f'  {name}: {t / base:.2f} x the parent kernel on the RGB frame')
    b0, b8 = med['image_to_nchw_alpha RGBA8 -> f16 opaque, bleed 0'], med['image_to_nchw_alpha RGBA8 -> f16 opaque, bleed 8']
    print(f'  expectation "opaque bleed 8 costs no more than bleed 0 plus the spread": bleed 8 median {b8[0]:.1f} us, bleed 0 median {b0[0]:.1f} us, '
          f'spread of bleed 0 (max - min) {b0[2] - b0[1]:.1f} us: {"confirmed" if b8[0] <= b0[0] + (b0[2] - b0[1]) else "REFUTED"}')  # fmt: skip

    big = (H * SCALE, W * SCALE)
    px = big[0] * big[1]
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (1, *big, 3), generator=g, dtype=torch.uint8).to(dev)
    x16 = ops.image_u8_to_nchw(img, torch.float16)
    a16 = x16[:, :1].contiguous()
    del img
    runs = {
        'nchw_to_image_u8 f16 -> RGB8 4320 x 7680 (parent)': (lambda: ops.nchw_to_image_u8(x16), px * (3 * 2 + 3)),
        'nchw_to_image_alpha f16 -> RGBA8, no alpha source': (lambda: ops.nchw_to_image_alpha(x16, None, 4, 8), px * (3 * 2 + 4)),
        'nchw_to_image_alpha f16 -> RGBA8, alpha from 1 channel': (lambda: ops.nchw_to_image_alpha(x16, a16, 4, 8), px * (4 * 2 + 4)),
        'nchw_to_image_alpha f16 -> RGBA8, alpha from 3 channels': (lambda: ops.nchw_to_image_alpha(x16, x16, 4, 8), px * (6 * 2 + 4)),
        'nchw_to_image_alpha f16 -> RGBA16, alpha from 1 channel': (lambda: ops.nchw_to_image_alpha(x16, a16, 4, 16), px * (4 * 2 + 8)),
        'nchw_to_image_alpha f16 -> RGB8': (lambda: ops.nchw_to_image_alpha(x16, None, 3, 8), px * (3 * 2 + 3)),
    }
    med = _timed(runs, n)
    base = med['nchw_to_image_u8 f16 -> RGB8 4320 x 7680 (parent)'][0]
    for name, (t, lo, hi) in med.items():
        if name.startswith('nchw_to_image_alpha'):
            print(f'  {name}: {t / base:.2f} x the parent kernel on the same frame')
    t = med['nchw_to_image_alpha f16 -> RGBA8, no alpha source'][0]
    print(f'  expectation "the RGBA8 launch costs no more than the parent\'s RGB kernel": {t:.1f} us against {base:.1f} us: {"confirmed" if t <= base else "REFUTED"}')


def frames(n):
    import time

    import torch

    import resselt_amd
    from resselt_amd import tiling
    from resselt_amd.utils import synth

    dev = torch.device('cuda:0')
    rrdb = resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=23, seed=0))).to(dev)
    compact = resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=64, num_conv=16, upscale=4, seed=0))).to(dev)
    opaque, holed = _frame(False)[0].to(dev), _frame(True)[0].to(dev)
    rgb = opaque[..., :3].contiguous()
    groups = {'RRDBNet (23 blocks), 2 x 2 tiles of (540, 960), halo 32': (rrdb, dict(tile=TILE, halo=HALO)), 'Compact (64 x 16) f16, untiled': (compact, {})}
    for title, (m, kw) in groups.items():
        variants = {
            'rgb: upscale() on the 8-bit RGB image': lambda: tiling.upscale(m, rgb, **kw),
            'rgba opaque: upscale_rgba()': lambda: tiling.upscale_rgba(m, opaque, **kw),
            "rgba 30 % transparent, alpha='model'": lambda: tiling.upscale_rgba(m, holed, alpha='model', **kw),
            "rgba 30 % transparent, alpha='resample'": lambda: tiling.upscale_rgba(m, holed, alpha='resample', **kw),
            'rgb again': lambda: tiling.upscale(m, rgb, **kw),
        }
        out = {}
        for _ in range(WARMUP):
            for name, run in variants.items():
                out[name] = tuple(run().shape)
        times = {name: [] for name in variants}
        for _ in range(n):
            for name, run in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                times[name].append((time.perf_counter() - t0) * 1e3)
        print(title)
        base = statistics.median(times['rgb: upscale() on the 8-bit RGB image'])
        for name, t in times.items():
            print(f'  {name} -> {out[name]}: median {statistics.median(t):.3f} ms/frame ({statistics.median(t) / base:.3f} x rgb), mean {statistics.mean(t):.3f}, '
                  f'min {min(t):.3f}, max {max(t):.3f}, stdev {statistics.stdev(t):.3f} over {n} frames alternated with the other variants')  # fmt: skip


if __name__ == '__main__':
    argv = sys.argv[1:]
    if not argv or argv[0] not in ('kernels', 'frames'):
        sys.exit(__doc__)
    if argv[0] == 'kernels':
        kernels(int(argv[1]) if len(argv) > 1 else 20)
    else:
        frames(int(argv[1]) if len(argv) > 1 else 8)
