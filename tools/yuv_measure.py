#!/usr/bin/env python3
"""What the video pixel formats of ``upscale_yuv`` cost at the size a user runs: a 1080 x 1920 NV12 / P010 frame in, the 4320 x 7680 frame of
RealESRGAN-x4plus (RRDBNet, 23 blocks) out (profiles/yuv_measure.txt).

  yuv_measure.py kernels [N]
      The launches alone, N of each (default 20) alternated after a warm-up, device events around each (the output allocation included):
      ``rsa_nchw_to_yuv420`` on the 4320 x 7680 f16 frame to NV12 and to P010 with both sitings, beside the parent's
      ``rsa_nchw_to_image_u8`` on the same frame; ``rsa_yuv420_to_nchw`` on a 1080 x 1920 frame from NV12 and P010 to f16, beside the
      parent's ``rsa_image_u8_to_nchw``.  Each with its byte model (every operand once) at 8 TB/s.
  yuv_measure.py frames [N]
      N frames (default 12) each of whole calls, alternated in one process after a warm-up, host clock around the call (every call ends in
      a device synchronise): ``upscale_yuv`` NV12 -> NV12 against ``upscale`` on the 8-bit RGB image of the same frame, for RRDBNet in 2 x 2
      tiles of (540, 960), halo 32, and for a Compact network (64 features, 16 convolutions, x4) untiled on f16 tensors; the RGB variant is
      timed twice (``rgb`` and ``rgb again``): their difference is the run-to-run spread.  And the same NV12 -> NV12 job with the chain of
      torch operations a caller needed before (the f32 torch form of the definition in engine/ops.py, run on the GPU) around the same model.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, SCALE, TILE, HALO = 1080, 1920, 4, (540, 960), 32
WARMUP = 2
BYTES_PER_S = 8e12  # what the project prices a byte at


def _timed(runs, n, unit):
    """``runs``: name -> (callable, byte model or None).  Alternates them ``n`` times between device events and prints one line each."""
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
        print(f'{name}: median {med:.1f} us between device events (min {min(t):.1f}, max {max(t):.1f}, {n} launches, includes the output allocation); '
              f'byte model {model / 1e6:.1f} MB = {model / BYTES_PER_S * 1e6:.1f} us at 8 TB/s: ratio {med * 1e-6 / (model / BYTES_PER_S):.2f}')  # fmt: skip
    return {name: statistics.median(t) for name, t in times.items()}


def kernels(n):
    import torch

    from resselt_amd.engine import ops

    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    big = (H * SCALE, W * SCALE)
    img = torch.randint(0, 256, (1, *big, 3), generator=g, dtype=torch.uint8).to(dev)
    x16 = ops.image_u8_to_nchw(img, torch.float16)
    px = big[0] * big[1]
    runs = {'nchw_to_image_u8 f16 4320 x 7680 (parent)': (lambda: ops.nchw_to_image_u8(x16), px * (3 * 2 + 3))}
    for fmt, e in (('nv12', 1), ('p010', 2)):
        for loc in ('left', 'center'):
            runs[f'nchw_to_yuv420 f16 -> {fmt} {loc} 4320 x 7680'] = (lambda f=fmt, c=loc: ops.nchw_to_yuv420(x16, f, chroma_loc=c), px * (3 * 2) + px * 3 // 2 * e)
    med = _timed(runs, n, 'us')
    base = med['nchw_to_image_u8 f16 4320 x 7680 (parent)']
    for name, t in med.items():
        if name.startswith('nchw_to_yuv420'):
            print(f'  {name}: {t / base:.2f} x the parent kernel on the same frame (expected: at most 1.25)')
    small = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    px = H * W
    runs = {'image_u8_to_nchw -> f16 1080 x 1920 (parent)': (lambda: ops.image_u8_to_nchw(small, torch.float16), px * (3 + 3 * 2))}
    planes = {}
    for fmt, e in (('nv12', 1), ('p010', 2)):
        planes[fmt] = ops.nchw_to_yuv420(ops.image_u8_to_nchw(small, torch.float16), fmt)
        for loc in ('left', 'center'):
            runs[f'yuv420_to_nchw {fmt} {loc} -> f16 1080 x 1920'] = (lambda f=fmt, c=loc: ops.yuv420_to_nchw(*planes[f], f, chroma_loc=c), px * 3 // 2 * e + px * 3 * 2)
    med = _timed(runs, n, 'us')
    base = med['image_u8_to_nchw -> f16 1080 x 1920 (parent)']
    for name, t in med.items():
        if name.startswith('yuv420_to_nchw'):
            print(f'  {name}: {t / base:.2f} x the parent kernel on the same frame')


def frames(n):
    import time

    import torch

    import resselt_amd
    from resselt_amd import tiling
    from resselt_amd.engine import ops
    from resselt_amd.utils import synth

    dev = torch.device('cuda:0')
    rrdb = resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=23, seed=0))).to(dev)
    compact = resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=64, num_conv=16, upscale=4, seed=0))).to(dev)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    y, uv = ops.nchw_to_yuv420(ops.image_u8_to_nchw(img, torch.float16))
    y, uv = y[0], uv[0]

    def torch_chain(m, kw):
        x = ops._yuv420_to_nchw_torch(y[None], uv[None], 8, 'bt709', 'limited', 'left', torch.float16)
        if 'tile' in kw:
            out = tiling.upscale_tiled(m, x, SCALE, kw['tile'], kw['halo'], check=False)
        else:
            out = m(x)
        planes = ops._nchw_to_yuv420_torch(out, 8, torch.uint8, 'bt709', 'limited', 'left')
        torch.cuda.synchronize()
        return planes[0]

    groups = {'RRDBNet (23 blocks), 2 x 2 tiles of (540, 960), halo 32': (rrdb, dict(tile=TILE, halo=HALO)), 'Compact (64 x 16) f16, untiled': (compact, {})}
    for title, (m, kw) in groups.items():
        variants = {
            'rgb: upscale() on the 8-bit RGB image': lambda: tiling.upscale(m, img, **kw),
            'yuv: upscale_yuv() NV12 -> NV12': lambda: tiling.upscale_yuv(m, y, uv, **kw)[0],
            'rgb again': lambda: tiling.upscale(m, img, **kw),
            'torch chain NV12 -> NV12 around the same model': lambda: torch_chain(m, kw),
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
        for name, t in times.items():
            print(f'  {name} -> {out[name]}: median {statistics.median(t):.3f} ms/frame, mean {statistics.mean(t):.3f}, min {min(t):.3f}, max {max(t):.3f}, '
                  f'stdev {statistics.stdev(t):.3f} over {n} frames alternated with the other variants')  # fmt: skip


if __name__ == '__main__':
    argv = sys.argv[1:]
    if not argv or argv[0] not in ('kernels', 'frames'):
        sys.exit(__doc__)
    if argv[0] == 'kernels':
        kernels(int(argv[1]) if len(argv) > 1 else 20)
    else:
        frames(int(argv[1]) if len(argv) > 1 else 12)
