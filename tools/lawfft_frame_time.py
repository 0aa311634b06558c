#!/usr/bin/env python3
"""Forward time of the default LAWFFT (x4, dim 60 = 15 local + 45 global, 4 x 6 blocks, pixelshuffledirect) on 1x3x512x512.  Run it under
``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/lawfft_frame_time.py`` for the per-kernel shares; ``--labels FILE``
writes the forward's priced launches (kernel, FLOP and byte model per frame), the file tools/lawfft_trace_summary.py holds a trace
against.  ``--wincorr`` times rsa_lawfft_wincorr alone instead, at hidden width 48 on 512 x 512 in the precision's plane form, beside the
time its byte model (q, k and v read once, the output written once) implies at 6.29 TB/s, the measured HBM copy rate of the MI355X.
usage: lawfft_frame_time.py [precision] [rounds] [size] [--labels FILE] [--wincorr]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.engine import lib as L  # noqa: E402
from resselt_amd.engine import lib_lawfft as LW  # noqa: E402
from resselt_amd.engine import ops  # noqa: E402
from resselt_amd.engine.base import PRECISIONS  # noqa: E402
from resselt_amd.engine.tensors import Planes  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402

HBM_COPY_RATE = 6.29e12  # bytes / s

args = [a for a in sys.argv[1:] if not a.startswith('--')]
labels = sys.argv[sys.argv.index('--labels') + 1] if '--labels' in sys.argv else None
if labels:
    args.remove(labels)
prec = args[0] if args else 'auto'
rounds = int(args[1]) if len(args) > 1 else 10
size = int(args[2]) if len(args) > 2 else 512
dev = torch.device('cuda:0')
WARMUP = 2


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return t


if '--wincorr' in sys.argv:
    C = 48
    products, fmt = PRECISIONS['bf16x3' if prec == 'auto' else prec]
    with_lo = products == 3
    gen = torch.Generator().manual_seed(0)
    D = Planes.empty(1, 3 * C // 8, size, size, dev, with_lo, fmt)
    D.hi.copy_(torch.randn(D.hi.shape, generator=gen).to(D.hi.dtype))
    if with_lo:
        D.lo.copy_((torch.randn(D.lo.shape, generator=gen) * 2.0**-9).to(D.lo.dtype))
    O = Planes.empty(1, C // 8, size, size, dev, with_lo, fmt)
    w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    p = LW.LawfftWincorrParams()
    p.batch, p.H, p.W, p.C, p.fmt, p.eps = 1, size, size, C, fmt, 1e-6
    p.weight, p.bias = w.data_ptr(), b.data_ptr()
    D.bind(p, 'q')
    D.bind(p, 'k', C // 8)
    D.bind(p, 'v', 2 * C // 8)
    O.bind(p, 'out')
    lib = L.load()

    def run():
        L.check(lib.rsa_lawfft_wincorr(ctypes.byref(p), ctypes.c_void_p(ops.current_stream_ptr(dev))), 'rsa_lawfft_wincorr')

    t = timed(run)
    nbytes = size * size * 4 * (C // 8) * 16 * (2 if with_lo else 1)
    model_us = nbytes / HBM_COPY_RATE * 1e6
    us = statistics.median(t) * 1e3
    print(f'rsa_lawfft_wincorr C {C} {size}x{size} {"bf16 hi + lo" if with_lo else "fp16 hi"}: {us:.1f} us (min {min(t) * 1e3:.1f}), byte model {nbytes / 1e6:.1f} MB = '
          f'{model_us:.1f} us at 6.29 TB/s: {us / model_us:.2f} x the model, {nbytes / us / 1e6:.2f} TB/s; {2 * 64 * size * size * C / us / 1e6:.1f} TFLOP/s of f32 FMA', flush=True)  # fmt: skip
    sys.exit(0)

x = synth.synth_input((1, 3, size, size), seed=0).to(dev)
name, sd = 'LAWFFT x4 d60 r4 m6', synth.lawfft_state_dict(scale=4, seed=0)
m = resselt_amd.load_from_state_dict(dict(sd)).to(dev)
m.precision = prec
t = timed(lambda: m(x))
y = m(x)
torch.cuda.synchronize()
print(f'{name} {m.resolved_precision()} {size}x{size}: {statistics.median(t):.3f} ms/frame (min {min(t):.3f}), out {tuple(y.shape)}, '
      f'{m.launches_per_forward()} launches, {rounds + WARMUP + 1} forwards', flush=True)  # fmt: skip
if labels:
    per = {}
    for meta, _ in m.last_plan().kernel_calls:
        k = per.setdefault(meta['kernel'], dict(launches=0, flop=0, bytes=0))
        k['launches'], k['flop'], k['bytes'] = k['launches'] + 1, k['flop'] + meta.get('flop', 0), k['bytes'] + meta.get('bytes', 0)
    with open(labels, 'w') as f:
        json.dump(dict(model=name, size=size, forwards=rounds + WARMUP + 1, warmup=WARMUP, frame_ms=statistics.median(t), kernels=per), f)
