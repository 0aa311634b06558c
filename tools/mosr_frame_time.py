#!/usr/bin/env python3
"""Forward time of MoSR x4 (24 blocks, dim 64, 'ps') and MoSRv2 x2 (defaults: unshuffle_mod, pixelshuffledirect) on 1x3x1080x1920.
Run it under ``rocprofv3 --kernel-trace --stats -- python tools/mosr_frame_time.py`` for the per-kernel shares (MoSR section).
usage: mosr_frame_time.py [precision] [rounds]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402

dev = torch.device('cuda:0')
prec = sys.argv[1] if len(sys.argv) > 1 else 'auto'
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
x = synth.synth_input((1, 3, 1080, 1920), seed=0).to(dev)
for name, sd in (('MoSR x4 d64 b24', synth.mosr_state_dict(upscale=4, n_block=24, dim=64, seed=0)),
                 ('MoSRv2 x2 d64 b24', synth.mosrv2_state_dict(scale=2, n_block=24, dim=64, seed=0))):  # fmt: skip
    m = resselt_amd.load_from_state_dict(dict(sd)).to(dev)
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
          f'{m.launches_per_forward()} launches', flush=True)  # fmt: skip
    del m, y
    torch.cuda.empty_cache()
