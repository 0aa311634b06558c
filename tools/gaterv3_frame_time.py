#!/usr/bin/env python3
"""Forward time of GateRV3 on one 1x3xSxS frame: the default x1 model ((2, 2, 4, 8) / (2, 2, 2, 2), 12 latent blocks, four span blocks)
and a x4 pixelshuffle one, with and without ``attention``, in 'bf16x3' and 'fp16'; GateR v1 (dim 48) is timed in the same run, for scale.
Every configuration is warmed up, then the rounds alternate between the configurations, so that a drift of the clocks lands on all of them
alike; the figure is the median over the rounds, the minimum beside it.  Run one configuration under
``rocprofv3 --kernel-trace --stats -- python tools/gaterv3_frame_time.py --only x1`` for the kernel table.
usage: gaterv3_frame_time.py [rounds] [size] [--only x1|x1_att|x4|x4_att|gater]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
if only:
    args.remove(only)
rounds = int(args[0]) if args else 10
size = int(args[1]) if len(args) > 1 else 512
dev = torch.device('cuda:0')
x = synth.synth_input((1, 3, size, size), seed=0).to(dev)
X4 = dict(scale=4, upsample='pixelshuffle', upsample_mid_dim=32)
CONFIGS = {
    'x1': ('GateRV3 x1 d32 default', lambda: synth.gaterv3_state_dict(seed=0)),
    'x1_att': ('GateRV3 x1 d32 attention', lambda: synth.gaterv3_state_dict(attention=True, seed=0)),
    'x4': ('GateRV3 x4 pixelshuffle d32', lambda: synth.gaterv3_state_dict(seed=0, **X4)),
    'x4_att': ('GateRV3 x4 pixelshuffle d32 attention', lambda: synth.gaterv3_state_dict(attention=True, seed=0, **X4)),
    'gater': ('GateR v1 d48', lambda: synth.gater_state_dict(seed=0)),
}
runs = []
for key, (name, make) in CONFIGS.items():
    if only and key != only:
        continue
    for prec in ('bf16x3', 'fp16'):
        m = resselt_amd.load_from_state_dict(dict(make())).to(dev)
        m.precision = prec
        for _ in range(2):
            y = m(x)
        torch.cuda.synchronize()
        runs.append((f'{name} {prec}', m, [], tuple(y.shape)))
for _ in range(rounds):
    for _, m, t, _ in runs:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m(x)
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
for name, m, t, shape in runs:
    print(f'{name} {size}x{size}: {statistics.median(t):.3f} ms/frame (min {min(t):.3f}, max {max(t):.3f}), out {shape}, {m.launches_per_forward()} launches, '
          f'{rounds} rounds alternated', flush=True)  # fmt: skip
