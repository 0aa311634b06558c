#!/usr/bin/env python3
"""What seam blending costs at the size a user runs: a 1080 x 1920 uint8 frame through RealESRGAN-x4plus (RRDBNet, 23 blocks) in 2 x 2
tiles of (540, 960) with a halo of 32 (profiles/tile_blend_measure.txt, DESIGN.md "Tile seams").

  tile_blend_measure.py frames [N] [--parent-tiling FILE]
      N frames (default 24) each of ``upscale(blend=16)`` and ``upscale(blend=0)``, alternated in one process after a warm-up of both, host
      clock around the call (``upscale`` ends in a device synchronise).  With ``--parent-tiling``, FILE -- a copy of resselt_amd/tiling.py
      from the parent commit -- is loaded beside this tree's and its ``upscale`` (no blend) is a third variant in the same alternation; its
      frame is compared with this tree's ``blend=0`` frame by ``torch.equal``.
  tile_blend_measure.py one VARIANT [N] [--parent-tiling FILE]
      N frames (default 5, after 2 warm-up frames) of one variant -- blend16, blend0 or parent0 -- for a run of its own under
      ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/tile_blend_measure.py one VARIANT``.
  tile_blend_measure.py stats DIR FRAMES
      The kernel dispatches per frame in the ``*_kernel_stats.csv`` under DIR, and the rows of the blending kernel beside its byte model.
"""
import csv
import glob
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, TILE, HALO, BLEND, SCALE = 1080, 1920, (540, 960), 32, 16, 4
WARMUP = 2
BYTES_PER_S = 8e12  # what the project prices a byte at


def byte_model():
    """(bytes, pixels) of the four launches of one frame: the source window once (1 B per value), 4 B per accumulator value written, 4 B
    per value of the top / left ramps read."""
    from resselt_amd.tiling import blend_window, plan_tiles

    total = 0
    for t in plan_tiles(H, W, -(-H // TILE[0]), -(-W // TILE[1]), HALO):
        py0, py1, px0, px1, top, _, left, _ = blend_window(t, H, W, BLEND, SCALE)
        wh, ww = py1 - py0, px1 - px0
        band = top * ww + (wh - top) * left
        total += 3 * (wh * ww * (1 + 4) + band * 4)
    return total


def setup(parent_file):
    import torch

    import resselt_amd
    from resselt_amd import tiling
    from resselt_amd.utils import synth

    dev = torch.device('cuda:0')
    m = resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=23, seed=0))).to(dev)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    variants = {
        'blend16': lambda: tiling.upscale(m, img, tile=TILE, halo=HALO, blend=BLEND),
        'blend0': lambda: tiling.upscale(m, img, tile=TILE, halo=HALO),
    }
    if parent_file:
        spec = importlib.util.spec_from_file_location('resselt_amd._parent_tiling', parent_file)
        parent = sys.modules[spec.name] = importlib.util.module_from_spec(spec)  # (dataclasses look their module up there)
        spec.loader.exec_module(parent)
        assert not hasattr(parent, 'blend_window')
        variants['parent0'] = lambda: parent.upscale(m, img, tile=TILE, halo=HALO)
    return variants


def frames(n, parent_file):
    import time

    import torch

    variants = setup(parent_file)
    out = {}
    for _ in range(WARMUP):
        for name, run in variants.items():
            out[name] = run()
    if 'parent0' in out:
        print(f'blend0 of this tree equals the parent\'s frame: {torch.equal(out["blend0"], out["parent0"])}')
    print(f'blend16 differs from blend0 at {int((out["blend16"] != out["blend0"]).sum())} of {out["blend0"].numel()} values')
    times = {name: [] for name in variants}
    for _ in range(n):
        for name, run in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, t in times.items():
        print(f'{name}: median {statistics.median(t):.3f} ms/frame, mean {statistics.mean(t):.3f}, min {min(t):.3f}, max {max(t):.3f}, '
              f'stdev {statistics.stdev(t):.3f} over {n} frames alternated with the other variants')  # fmt: skip
    b = byte_model()
    print(f'byte model of the four blending launches of a frame: {b / 1e6:.1f} MB = {b / BYTES_PER_S * 1e6:.1f} us at 8 TB/s')


def one(variant, n, parent_file):
    run = setup(parent_file)[variant]
    for _ in range(WARMUP + n):
        run()
    print(f'{variant}: {WARMUP + n} frames')


def stats(folder, n_frames):
    files = glob.glob(os.path.join(folder, '**', '*kernel_stats.csv'), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    calls = sum(int(r['Calls']) for r in rows)
    print(f'{folder}: {calls} kernel dispatches in {n_frames} frames = {calls / n_frames:.2f} per frame, {len(rows)} kernel names')
    b = byte_model()
    for r in rows:
        if 'tile_blend' in r['Name']:
            avg = float(r['TotalDurationNs']) / int(r['Calls'])
            print(f'  {r["Name"][:90]}: {r["Calls"]} calls, mean {avg / 1e3:.1f} us (min {float(r["MinNs"]) / 1e3:.1f}, max {float(r["MaxNs"]) / 1e3:.1f}); '
                  f'byte model {b / 4 / 1e6:.1f} MB per launch = {b / 4 / BYTES_PER_S * 1e6:.1f} us at 8 TB/s: ratio {avg * 1e-9 / (b / 4 / BYTES_PER_S):.2f}')  # fmt: skip


if __name__ == '__main__':
    argv = sys.argv[1:]
    parent_file = None
    if '--parent-tiling' in argv:
        i = argv.index('--parent-tiling')
        parent_file = argv[i + 1]
        del argv[i : i + 2]
    if argv[0] == 'frames':
        frames(int(argv[1]) if len(argv) > 1 else 24, parent_file)
    elif argv[0] == 'one':
        one(argv[1], int(argv[2]) if len(argv) > 2 else 5, parent_file)
    elif argv[0] == 'stats':
        stats(argv[1], int(argv[2]))
    else:
        sys.exit(__doc__)
