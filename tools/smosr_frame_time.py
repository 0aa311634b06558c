#!/usr/bin/env python3
"""Forward time of SMoSR (dim 48, 3 + 3 + 1 blocks: the defaults) on 1x3x512x512, x2 or x4, with the default pixelshuffledirect head or
with pa_up (mid_dim 32).  Run it under ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/smosr_frame_time.py x2_pa``
for the per-kernel shares; ``--labels FILE`` writes the forward's rsa_smosr_gate and rsa_smosr_pa launches in launch order (what each
reads and writes, map size, byte model) for tools/smosr_trace_summary.py to attach to the trace's dispatches.
usage: smosr_frame_time.py x2|x4|x2_pa|x4_pa [precision] [rounds] [--labels FILE]"""
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
which = args[0] if args else 'x2'
prec = args[1] if len(args) > 1 else 'auto'
rounds = int(args[2]) if len(args) > 2 else 20
dev = torch.device('cuda:0')
x = synth.synth_input((1, 3, 512, 512), seed=0).to(dev)
scale = 4 if which.startswith('x4') else 2
head = dict(upsampler='pa_up', upsampler_mid_dim=32) if which.endswith('_pa') else {}
name = f'SMoSR x{scale} d48 {"pa_up m32" if head else "pixelshuffledirect"}'
m = resselt_amd.load_from_state_dict(dict(synth.smosr_state_dict(scale=scale, seed=0, **head))).to(dev)
m.precision = prec
for _ in range(3):
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
print(f'{name} {m.resolved_precision()}: {statistics.median(t):.3f} ms/frame (min {min(t):.3f}), out {tuple(y.shape)}, '
      f'{m.launches_per_forward()} launches, {rounds + 3} forwards', flush=True)  # fmt: skip
if labels:
    calls = [meta for meta, _ in m.last_plan().kernel_calls if meta['kernel'] in ('rsa_smosr_gate', 'rsa_smosr_pa')]
    with open(labels, 'w') as f:
        json.dump(dict(model=name, forwards=rounds + 3, warmup=3, launches=[dict(kernel=c['kernel'], label=c['label'], bytes=c['bytes']) for c in calls]), f)
