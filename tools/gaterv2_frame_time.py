#!/usr/bin/env python3
"""Forward time of GateRv2 on one 1x3xSxS frame: the default x1 model (dim 48, (2, 2, 4, 6) / (2, 2, 2, 2), 10 latent blocks at 768
channels) and a x4 pixelshuffle one, in 'bf16x3' and 'fp16'; GateRV3 (attention on) and GateR v1 (dim 48) are timed in the same run, for
scale.  Every configuration is warmed up, then the rounds alternate between the configurations, so that a drift of the clocks lands on all
of them alike; the figure is the median over the rounds, the minimum beside it.  ``--attention`` also prints, per model with the kernel, the
launches' own time of rsa_gaterv2_linear_attention (events around replays of its recorded launches) against its byte model.  Run one
configuration under ``rocprofv3 --kernel-trace --stats -- python tools/gaterv2_frame_time.py --only x1`` for the kernel table.
usage: gaterv2_frame_time.py [rounds] [size] [--only x1|x4|gaterv3_att|gater] [--attention]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402

flags = [a for a in sys.argv[1:] if a.startswith('--')]
args = [a for a in sys.argv[1:] if not a.startswith('--')]
only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
if only:
    args.remove(only)
rounds = int(args[0]) if args else 10
size = int(args[1]) if len(args) > 1 else 512
dev = torch.device('cuda:0')
x = synth.synth_input((1, 3, size, size), seed=0).to(dev)
CONFIGS = {
    'x1': ('GateRv2 x1 d48 default', lambda: synth.gaterv2_state_dict(seed=0)),
    'x4': ('GateRv2 x4 pixelshuffle d48', lambda: synth.gaterv2_state_dict(seed=0, scale=4, upsample='pixelshuffle', upsample_mid_dim=32)),
    'gaterv3_att': ('GateRV3 x1 d32 attention', lambda: synth.gaterv3_state_dict(attention=True, seed=0)),
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
if '--attention' in flags:
    for name, m, _, _ in runs:
        calls = [(meta, fn) for meta, fn in m.last_plan().kernel_calls if meta['kernel'] == 'rsa_gaterv2_linear_attention']
        if not calls:
            continue
        times = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _, fn in calls:
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        nbytes = sum(meta['bytes'] for meta, _ in calls)
        med = statistics.median(times)
        print(f'{name}: rsa_gaterv2_linear_attention x {len(calls)} (3 kernels each, back to back): {1e3 * med / len(calls):.1f} us per call (min '
              f'{1e3 * min(times) / len(calls):.1f}), byte model {nbytes / len(calls) / 1e6:.3f} MB per call = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s', flush=True)  # fmt: skip
