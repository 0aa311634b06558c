#!/usr/bin/env python3
"""What ``upscale(out_scale=)`` costs at the size a user runs: the 4320 x 7680 x 3 native frame of a 1080 x 1920 uint8 frame through
RealESRGAN-x4plus (RRDBNet, 23 blocks), delivered at x2 (2160 x 3840) and x3 (3240 x 5760) (profiles/resample_measure.txt).

  resample_measure.py kernels [N]
      The launches alone, N of each (default 20) alternated after a warm-up, device events around each: ``rsa_resample`` to an 8-bit image at
      ``out_scale`` 2 and 3, bicubic, from the frame as an f16 NCHW tensor (the float path), as an f32 NCHW tensor (a blend's accumulator)
      and as the model's own 8-bit image (RRDBNet's path); and the parent's ``rsa_nchw_to_image_u8`` on the f16 and f32 frames.  Each with
      its byte model (source once + destination once).  Run it under ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
      python tools/resample_measure.py kernels`` for kernel times, then ``stats DIR``.
  resample_measure.py frames [N]
      N frames (default 16) each of whole ``upscale()`` calls with and without ``out_scale=2``, alternated in one process after a warm-up,
      host clock around the call (``upscale`` ends in a device synchronise): RRDBNet in 2 x 2 tiles of (540, 960), halo 32, hard crop and
      ``blend=16``; and a Compact network (64 features, 16 convolutions, x4) untiled on f16 tensors, where the resample launch takes the place
      of the conversion kernel.  The same variant is timed twice (``plain`` and ``plain again``): their difference is the run-to-run spread.
  resample_measure.py stats DIR
      Per kernel name and grid of the ``*_kernel_trace.csv`` under DIR: dispatches, mean / min / max duration, and for the two kernels above
      the byte model and duration / byte model.
"""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, SCALE, TILE, HALO, BLEND = 1080, 1920, 4, (540, 960), 32, 16
NATIVE = (H * SCALE, W * SCALE)
WARMUP = 2
BYTES_PER_S = 8e12  # what the project prices a byte at
ELEM = {'f16': 2, 'f32': 4, 'u8': 1}


def target(out_scale):
    return H * out_scale, W * out_scale


def byte_model(src_fmt, size):
    """Bytes of one launch: the native frame once in ``src_fmt``, the 8-bit image of ``size`` once."""
    return 3 * (NATIVE[0] * NATIVE[1] * ELEM[src_fmt] + size[0] * size[1])


def grid_of(size):
    """(x, y) workgroups of the resample launch for an output of ``size`` (16 x 64 tiles)."""
    return -(-size[1] // 64), -(-size[0] // 16)


def kernels(n):
    import torch

    from resselt_amd.engine import ops

    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (1, *NATIVE, 3), generator=g, dtype=torch.uint8).to(dev)
    frames = {'u8': img, 'f16': ops.image_u8_to_nchw(img, torch.float16), 'f32': ops.image_u8_to_nchw(img, torch.float32)}
    runs = {}
    for fmt in ('f16', 'f32', 'u8'):
        for s in (2, 3):
            runs[f'resample {fmt} -> u8 x{s}'] = (lambda f=fmt, s=s: ops.resample_to_image_u8(frames[f], target(s)), byte_model(fmt, target(s)))
    for fmt in ('f16', 'f32'):
        runs[f'nchw_to_image_u8 {fmt} (native size)'] = (lambda f=fmt: ops.nchw_to_image_u8(frames[f]), byte_model(fmt, NATIVE))
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


def frames(n):
    import time

    import torch

    import resselt_amd
    from resselt_amd import tiling
    from resselt_amd.utils import synth

    dev = torch.device('cuda:0')
    rrdb = resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=23, seed=0))).to(dev)
    compact = resselt_amd.load_from_state_dict(dict(synth.compact_state_dict(num_feat=64, num_conv=16, upscale=4, seed=0))).to(dev)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    groups = {
        'RRDBNet 8-bit, 2 x 2 tiles, hard crop': dict(model=rrdb, tile=TILE, halo=HALO),
        'RRDBNet 8-bit, 2 x 2 tiles, blend 16': dict(model=rrdb, tile=TILE, halo=HALO, blend=BLEND),
        'Compact f16, untiled': dict(model=compact, dtype=torch.float16),
    }
    for title, kw in groups.items():
        kw = dict(kw)
        m = kw.pop('model')
        variants = {
            'plain': lambda: tiling.upscale(m, img, **kw),
            'out_scale=2': lambda: tiling.upscale(m, img, out_scale=2, **kw),
            'plain again': lambda: tiling.upscale(m, img, **kw),
            'out_scale=3': lambda: tiling.upscale(m, img, out_scale=3, **kw),
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


def stats(folder):
    files = glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    by = {}
    for r in rows:
        name = r.get('Kernel_Name', '')
        if 'resample_kernel' not in name and 'nchw_to_image_u8' not in name:
            continue
        wg = (int(r.get('Workgroup_Size_X') or 1), int(r.get('Workgroup_Size_Y') or 1))
        grid = (int(r.get('Grid_Size_X') or 0) // wg[0], int(r.get('Grid_Size_Y') or 0) // wg[1])
        by.setdefault((name, grid), []).append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    print(f'{folder}: {len(rows)} kernel dispatches')
    models = {grid_of(target(s)): s for s in (2, 3)}

    def report(label, t, b):
        t = t[WARMUP:]  # the warm-up launches come first
        mean = statistics.mean(t)
        print(f'  {label}: {len(t)} dispatches, mean {mean / 1e3:.1f} us (min {min(t) / 1e3:.1f}, max {max(t) / 1e3:.1f}); byte model {b / 1e6:.1f} MB = '
              f'{b / BYTES_PER_S * 1e6:.1f} us at 8 TB/s: ratio {mean * 1e-9 / (b / BYTES_PER_S):.2f}')  # fmt: skip

    for (name, grid), t in sorted(by.items()):
        t = [d for _, d in sorted(t)]  # in launch order
        if 'resample_kernel' in name and grid in models:
            src = name.split('resample_kernel', 1)[1]
            fmt = 'f16' if src.startswith(('<_Float16', 'IDF16_')) else 'u8' if src.startswith(('<unsigned char', 'Ih')) else 'f32'
            report(f'resample {fmt} -> u8 x{models[grid]}, grid {grid} ({name[:70]})', t, byte_model(fmt, target(models[grid])))
        elif 'nchw_to_image_u8' in name:  # one kernel for every dtype: `kernels` launches it on the f16 and the f32 frame in turn
            report(f'nchw_to_image_u8 f16 (native size), grid {grid}', t[0::2], byte_model('f16', NATIVE))
            report(f'nchw_to_image_u8 f32 (native size), grid {grid}', t[1::2], byte_model('f32', NATIVE))
        else:
            print(f'  {name[:100]} grid {grid}: {len(t)} dispatches, mean {statistics.mean(t) / 1e3:.1f} us')


if __name__ == '__main__':
    argv = sys.argv[1:]
    if not argv:
        sys.exit(__doc__)
    if argv[0] == 'kernels':
        kernels(int(argv[1]) if len(argv) > 1 else 20)
    elif argv[0] == 'frames':
        frames(int(argv[1]) if len(argv) > 1 else 16)
    elif argv[0] == 'stats':
        stats(argv[1])
    else:
        sys.exit(__doc__)
