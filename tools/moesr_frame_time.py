#!/usr/bin/env python3
"""Forward time of the default MoESR x4 (dim 64, 9 x (4 + 3) gated blocks) or of MoSRv2 x4 (dim 64, 24 blocks, no unshuffle: the same
512 x 512 map) on 1x3x512x512.  Run it under ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/moesr_frame_time.py
moesr`` for the per-kernel shares; ``--labels FILE`` writes the forward's rsa_moesr_stream launches in launch order (mode, what the planes
hold, map size, byte model) for tools/moesr_trace_summary.py to attach to the trace's dispatches.
usage: moesr_frame_time.py moesr|mosrv2 [precision] [rounds] [--labels FILE]"""
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
which = args[0] if args else 'moesr'
prec = args[1] if len(args) > 1 else 'auto'
rounds = int(args[2]) if len(args) > 2 else 5
dev = torch.device('cuda:0')
x = synth.synth_input((1, 3, 512, 512), seed=0).to(dev)
name, sd = {'moesr': ('MoESR x4 d64 9x(4+3)', lambda: synth.moesr_state_dict(seed=0)),
            'mosrv2': ('MoSRv2 x4 d64 b24', lambda: synth.mosrv2_state_dict(scale=4, n_block=24, dim=64, seed=0))}[which]  # fmt: skip
m = resselt_amd.load_from_state_dict(dict(sd())).to(dev)
m.precision = prec
for _ in range(2):
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
print(f'{name} {m.resolved_precision()}: {statistics.median(t):.2f} ms/frame (min {min(t):.2f}), out {tuple(y.shape)}, '
      f'{m.launches_per_forward()} launches, {rounds + 2} forwards', flush=True)  # fmt: skip
if labels:
    calls = [meta for meta, _ in m.last_plan().kernel_calls if meta['kernel'] == 'rsa_moesr_stream']
    with open(labels, 'w') as f:
        json.dump(dict(model=name, forwards=rounds + 2, launches=[dict(label=c['label'], bytes=c['bytes']) for c in calls]), f)
