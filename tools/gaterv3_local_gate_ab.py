#!/usr/bin/env python3
"""rsa_gaterv3_local_gate against the unfused route's floor, alternated in one run: the same layer (MetaGated.local's grouped 3x3, 2 in /
2 out per group) as ONE zero-embedded dense rsa_conv2d over the 2 dim channels -- which does no gate and no pooling, so the unfused route
cannot be faster than it.  Kernel time = the time between two events around ``reps`` back-to-back launches, divided by ``reps`` (so it
includes the launch boundary); the rounds alternate fused / dense.  The byte model is what the fused kernel must read and write -- the
2 dim / 8 input planes once, the dim / 8 output planes once, hi and lo, plus a tile-sum record -- over the 8.0 TB/s HBM peak.
usage: gaterv3_local_gate_ab.py [rounds] [reps]   (dim 32 on 512 x 512 and dim 128 on 128 x 128, bf16 hi + lo planes)"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from resselt_amd.engine import lib as L  # noqa: E402
from resselt_amd.engine import lib_gaterv3 as LG3  # noqa: E402
from resselt_amd.engine import ops  # noqa: E402
from resselt_amd.engine.base import Prec  # noqa: E402
from resselt_amd.engine.tensors import Planes  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
PEAK = 8.0e12
dev = torch.device('cuda:0')
lib = L.load()
gen = torch.Generator().manual_seed(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per launch


for dim, side in ((32, 512), (128, 128)):
    n, H, W = 1, side, side
    x = Planes.empty(n, 2 * dim // 8, H, W, dev, True)
    x.hi.copy_(torch.randn(x.hi.shape, generator=gen).to(x.hi.dtype))
    x.lo.copy_((torch.randn(x.lo.shape, generator=gen) * 2.0**-9).to(x.lo.dtype))
    w = torch.randn(2 * dim, 2, 3, 3, generator=gen) / 18**0.5
    b = 0.1 * torch.randn(2 * dim, generator=gen)
    s = Planes.empty(n, dim // 8, H, W, dev, True)
    nbytes = lib.rsa_gaterv3_local_workspace_bytes(n, H, W, dim)
    ws = torch.empty(nbytes // 4, device=dev)
    wd, bd = w.reshape(2 * dim, 18).to(dev).contiguous(), b.to(dev)
    p = LG3.LocalGateParams()
    p.batch, p.H, p.W, p.dim, p.fmt = n, H, W, dim, x.fmt
    x.bind(p, 'x')
    s.bind(p, 'out')
    p.weight, p.bias, p.workspace, p.workspace_bytes = wd.data_ptr(), bd.data_ptr(), ws.data_ptr(), nbytes
    stream = C.c_void_p(ops.current_stream_ptr(dev))

    def fused(p=p, stream=stream):
        L.check(lib.rsa_gaterv3_local_gate(C.byref(p), stream), 'rsa_gaterv3_local_gate')

    dense_w = torch.zeros(2 * dim, 2 * dim, 3, 3)
    for o in range(2 * dim):
        dense_w[o, 2 * (o // 2) : 2 * (o // 2) + 2] = w[o]
    cw = ops.ConvWeights.from_oihw(dense_w, b, Prec('bf16x3'), device=dev)
    full = Planes.empty(n, 2 * dim // 8, H, W, dev, True)
    cp = [ops.conv_params(cw, x, H, W, out=full)]

    def dense(cp=cp):
        ops.run_convs(cp, dev)

    for fn in (fused, dense):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    tf, td = [], []
    for _ in range(rounds):
        tf.append(timed(fused))
        td.append(timed(dense))
    tiles = -(-H // LG3.TILE_H) * -(-W // LG3.TILE_W)
    model_bytes = n * H * W * (3 * dim // 8) * 32 + n * tiles * dim * 4
    model_us = model_bytes / PEAK * 1e6
    mf, md = statistics.median(tf), statistics.median(td)
    print(f'dim {dim} {H}x{W} bf16 hi+lo: rsa_gaterv3_local_gate {mf:.1f} us (min {min(tf):.1f}, max {max(tf):.1f}); byte model {model_bytes / 1e6:.1f} MB = '
          f'{model_us:.1f} us at 8.0 TB/s: time / model = {mf / model_us:.2f}; dense zero-embedded rsa_conv2d [{L.conv_kernel_name(cp[0])}] {md:.1f} us '
          f'(min {min(td):.1f}, max {max(td):.1f}): fused / dense = {mf / md:.2f}; {rounds} rounds alternated, {reps} launches each', flush=True)  # fmt: skip
