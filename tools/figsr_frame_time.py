#!/usr/bin/env python3
"""Forward time of the default FIGSR (x4, dim 48, 24 blocks, gc 8, 13x13 / 17 bands, pixelshuffledirect) on 1x3x512x512 (520x520 after
the model's own padding).  Run it under ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/figsr_frame_time.py``
for the per-kernel shares; ``--labels FILE`` writes the forward's priced launches (kernel, FLOP and byte model per frame), the file
tools/gfisrv2_trace_summary.py holds a trace against.
usage: figsr_frame_time.py [precision] [rounds] [size] [--labels FILE]"""
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
prec = args[0] if args else 'auto'
rounds = int(args[1]) if len(args) > 1 else 10
size = int(args[2]) if len(args) > 2 else 512
dev = torch.device('cuda:0')
x = synth.synth_input((1, 3, size, size), seed=0).to(dev)
name, sd = 'FIGSR x4 d48 b24', synth.figsr_state_dict(scale=4, seed=0)
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
