#!/usr/bin/env python3
"""Forward time of the default GFISR v1 (x4, dim 48, 24 blocks, pixelshuffledirect) on 1x3x512x512, or of the default GFISRv2 (the
yardstick: the same frame with v2's wider FourierUnit, dim - 3 gc = 30 channels against v1's gc = 6) on the same input.  Run it under
``rocprofv3 --kernel-trace --output-format csv -- python tools/gfisr_frame_time.py gfisr`` for the per-kernel shares; ``--labels FILE``
writes the forward's priced launches (kernel, FLOP and byte model per frame) for tools/gfisrv2_trace_summary.py to hold the trace against.
usage: gfisr_frame_time.py gfisr|gfisr_nofft|gfisrv2 [precision] [rounds] [size] [--labels FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
labels = sys.argv[sys.argv.index('--labels') + 1] if '--labels' in sys.argv else None
if labels:
    args.remove(labels)
which = args[0] if args else 'gfisr'
prec = args[1] if len(args) > 1 else 'auto'
rounds = int(args[2]) if len(args) > 2 else 10
size = int(args[3]) if len(args) > 3 else 512
dev = torch.device('cuda:0')
x = synth.synth_input((1, 3, size, size), seed=0).to(dev)
if which == 'gfisrv2':
    name, sd = 'GFISRv2 x4 d48 b24', synth.gfisrv2_state_dict(scale=4, seed=0)
elif which == 'gfisr_nofft':
    name, sd = 'GFISR x4 d48 b24 fft_mode=False', synth.gfisr_state_dict(scale=4, fft_mode=False, seed=0)
else:
    name, sd = 'GFISR x4 d48 b24', synth.gfisr_state_dict(scale=4, seed=0)
m = resselt_amd.load_from_state_dict(dict(sd)).to(dev)
m.precision = prec
WARMUP = 2
for _ in range(WARMUP):
    m(x)
torch.cuda.synchronize()
t = []
for _ in range(rounds):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    y = m(x)
    b.record()
    torch.cuda.synchronize()
    t.append(a.elapsed_time(b))
print(f'{name} {m.resolved_precision()} {size}x{size}: {statistics.median(t):.3f} ms/frame (min {min(t):.3f}), out {tuple(y.shape)}, '
      f'{m.launches_per_forward()} launches, {rounds + WARMUP} forwards', flush=True)  # fmt: skip
if labels:
    per = {}
    for meta, _ in m.last_plan().kernel_calls:
        k = per.setdefault(meta['kernel'], dict(launches=0, flop=0, bytes=0))
        k['launches'], k['flop'], k['bytes'] = k['launches'] + 1, k['flop'] + meta.get('flop', 0), k['bytes'] + meta.get('bytes', 0)
    with open(labels, 'w') as f:
        json.dump(dict(model=name, size=size, forwards=rounds + WARMUP, warmup=WARMUP, frame_ms=statistics.median(t), kernels=per), f)
