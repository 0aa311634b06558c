#!/usr/bin/env python3
"""Phase accounting of conv5 of a residual dense block on the coded residual stream (conv_ring.h XRES 4) on a diagnostic build
(tools/variant.sh c5_stamps "-DRSA_C5_STAMPS" conv_inst_ring1h; add -DRSA_C5_EPI=0 for the generic epilogue the kernel had before
epilogue_c5): per-wave s_memtime totals of one launch at 1080p, medians over the compute waves of the 256 workgroups.

columns: per tile, in microseconds (s_memtime ticks scaled so that a wave's lifetime is the launch time): full = waiting for ring fills (FULL), res = the epilogue waiting for a
step's residual data (the counted vmcnt made explicit), epi = the rest of the epilogue, mult = the K loop (what remains of the lifetime).
The stamped build is slower than the product (every stamp drains the scalar memory counter); the columns are for comparing builds.
usage: RSA_LIB=variants/lib_c5_stamps.so c5_stamps.py
"""

import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from resselt_amd.engine import lib as L  # noqa: E402

_p = os.path.abspath(os.environ['RSA_LIB'])
L.lib_path = lambda: _p
from resselt_amd.engine import ops, tensors  # noqa: E402

dev = torch.device('cuda:0')
lib = L.load()
raw = C.CDLL(_p)
raw.rsa_debug_c5_stamps.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
H, W, cin, cout = 1080, 1920, 192, 64
wts = ops.ConvWeights.from_oihw((torch.rand((cout, cin, 3, 3)) - 0.5) * 0.1, torch.zeros(cout), 1, device=dev, fmt=tensors.PF_F16)
mk = lambda: tensors.Planes.empty(1, cin // 8, H, W, dev, True, tensors.PF_F16, lo_planes=8).with_lo8(8)  # noqa: E731
x, r2, out = mk(), mk(), mk()
for t in (x, r2):
    t.hi.copy_(torch.randn(t.hi.shape, device=dev).to(torch.float16))
    t.lo8.copy_(torch.randint(0, 256, t.lo8.shape, device=dev, dtype=torch.uint8))
stream = ops.current_stream_ptr(dev)
print(os.environ['RSA_LIB'])
for two in (False, True):
    kw = dict(res2=(r2, 0, 'lo8'), beta=0.2) if two else {}
    p = ops.conv_params(wts, x, H, W, out=out, res1=(x, 0, 'lo8'), alpha=0.2, out_lo8=True, **kw)
    arr = (L.ConvParams * 1)(p)
    for _ in range(5):
        L.conv2d_list(arr, stream)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * (256 * 8 * 8))()
    raw.rsa_debug_c5_stamps(buf, len(buf))  # clear
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.conv2d_list(arr, stream)
    e1.record()
    torch.cuda.synchronize()
    raw.rsa_debug_c5_stamps(buf, len(buf))
    v = list(buf)
    rows = [v[i * 8 : i * 8 + 5] for i in range(256 * 8) if v[i * 8] > 0 and v[i * 8 + 4] > 0]
    launch = e0.elapsed_time(e1) * 1e3
    tiles = statistics.median(r[4] for r in rows)
    tick = launch / statistics.median(r[0] for r in rows)  # s_memtime ticks -> us: a wave lives for the whole launch
    us = lambda i: statistics.median(r[i] / r[4] for r in rows) * tick  # noqa: E731
    mult = statistics.median((r[0] - r[1] - r[3]) / r[4] for r in rows) * tick
    epi = statistics.median((r[3] - r[2]) / r[4] for r in rows) * tick
    print(f'  {"two residuals" if two else "one residual":13s} launch {launch:6.1f} us (stamped build), {len(rows)} waves, {tiles:.0f} tiles each;'
          f' per tile: {us(0):5.2f} us = mult {mult:5.2f} + full {us(1):5.2f} + res {us(2):5.2f} + epi {epi:5.2f}   aborts={L.ring_aborts()}')
