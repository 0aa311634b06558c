#!/usr/bin/env python3
"""rsa_figsr_mix against the composition it replaces, in one process on the same operands: two rsa_plk_conv launches with each band
embedded in a zero K x K kernel, then rsa_gfisr_gate over all planes.  The default FIGSR block at 512x512: hidden 128 (16 planes, 13
passed through, gc 8), K 17, a 520x520 map, batch 1.  The two are timed alternately with device events, ``reps`` launches per window,
after a warm-up of both; the median window of each is printed with the byte model of the fused kernel (resselt_amd/csrc/figsr.hip) and
the largest difference between the two results.
usage: figsr_mix_ab.py [bf16x3|fp16] [windows] [reps] [size]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from resselt_amd.engine import lib as L  # noqa: E402
from resselt_amd.engine import lib_figsr as LF  # noqa: E402
from resselt_amd.engine import lib_gfisr  # noqa: E402, F401  (registers rsa_gfisr_gate)
from resselt_amd.engine import ops, plk  # noqa: E402
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else 'bf16x3'
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 15
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
size = int(sys.argv[4]) if len(sys.argv) > 4 else 520
fmt, products, with_lo = (PF_BF16, 3, True) if mode == 'bf16x3' else (PF_F16, 1, False)
dev = torch.device('cuda:0')
H = W = size
K, GC, PLANES, PASS = 17, 8, 16, 13
gen = torch.Generator().manual_seed(0)


def planes_of(t):
    p = Planes.empty(1, t.shape[1] // 8, H, W, dev, with_lo, fmt)
    ops.nchw_to_planes(t.to(dev), p)
    return p


G = planes_of(torch.randn(1, 8 * PLANES, H, W, generator=gen))
X = planes_of(torch.randn(1, 8 * PLANES, H, W, generator=gen))
HW = planes_of(torch.randn(1, GC, H, W, generator=gen))
w_w, w_h = torch.randn(GC, GC, 1, K, generator=gen) / (GC * K) ** 0.5, torch.randn(GC, GC, K, 1, generator=gen) / (GC * K) ** 0.5
b_w, b_h = 0.1 * torch.randn(GC, generator=gen), 0.1 * torch.randn(GC, generator=gen)
stream = ops.current_stream_ptr(dev)

# the fused kernel
blob, bias_w, bias_h = LF.pack_band_weights(w_w, w_h, products, fmt).to(dev), LF.band_bias(b_w).to(dev), LF.band_bias(b_h).to(dev)
OUT_F = Planes.empty(1, PLANES, H, W, dev, with_lo, fmt)
mp = LF.FigsrMixParams()
mp.batch, mp.H, mp.W, mp.fmt, mp.products, mp.ksize, mp.gc, mp.planes, mp.pass_planes = 1, H, W, fmt, products, K, GC, PLANES, PASS
mp.w_packed, mp.bias_w, mp.bias_h = blob.data_ptr(), bias_w.data_ptr(), bias_h.data_ptr()
G.bind(mp, 'g')
X.bind(mp, 'x')
HW.bind(mp, 'hw')
OUT_F.bind(mp, 'out')

# the composition: cat = [x's passed planes | hw | plk(band w) | plk(band h)], then the gate over all of it
CAT = Planes.empty(1, PLANES, H, W, dev, with_lo, fmt)
CAT.hi[:, :PASS] = X.hi[:, :PASS]
CAT.hi[:, PASS : PASS + 1] = HW.hi
if with_lo:
    CAT.lo[:, :PASS] = X.lo[:, :PASS]
    CAT.lo[:, PASS : PASS + 1] = HW.lo
plks, keep = [], []
for band, (wt, bt) in enumerate(((w_w, b_w), (w_h, b_h))):
    full = torch.zeros(GC, GC, K, K)
    if band == 0:
        full[:, :, K // 2, :] = wt[:, :, 0, :]
    else:
        full[:, :, :, K // 2] = wt[:, :, :, 0]
    pb, bb = plk.pack_plk_weights(full.to(dev), products, fmt), plk.plk_bias(bt.to(dev))
    a = PASS + 1 + band
    src = Planes(X.hi[:, a : a + 1], None if X.lo is None else X.lo[:, a : a + 1])
    plks.append(plk.plk_params(pb, bb, K, products, src, CAT, a))
    keep += [pb, bb]
OUT_C = Planes.empty(1, PLANES, H, W, dev, with_lo, fmt)
gp = L.GatedDwConvParams()
gp.batch, gp.H, gp.W, gp.fmt, gp.i_planes, gp.n_segments = 1, H, W, fmt, PLANES, 0
G.bind(gp, 'g')
CAT.bind(gp, 'x')
OUT_C.bind(gp, 'out')


def fused():
    L.launch('rsa_figsr_mix', mp, stream)


def composed():
    for p in plks:
        L.launch('rsa_plk_conv', p, stream)
    L.invoke('rsa_gfisr_gate', [gp, L.ACT_SILU], stream)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # microseconds per call


for fn in (fused, composed):
    for _ in range(3):
        fn()
torch.cuda.synchronize()
L.check_status('figsr_mix_ab')
value = lambda p: p.hi.double() + (p.lo.double() if p.lo is not None else 0.0)  # noqa: E731
diff = (value(OUT_F) - value(OUT_C)).abs().max().item()
scale = value(OUT_C).abs().max().item()
tf, tc = [], []
for _ in range(windows):  # alternating windows: whatever else the machine does meets both
    tf.append(window(fused))
    tc.append(window(composed))
unit = 16 * (2 if with_lo else 1)
nbytes = H * W * unit * (PLANES + (PLANES - 1) + 1 + PLANES)  # g, x without its c_hw plane, hw, out
mf, mc = statistics.median(tf), statistics.median(tc)
print(f'figsr_mix A/B {mode} {H}x{W} hidden {8 * PLANES} gc {GC} K {K}: fused {mf:.1f} us (min {min(tf):.1f}, max {max(tf):.1f}), '
      f'2 x rsa_plk_conv + rsa_gfisr_gate {mc:.1f} us (min {min(tc):.1f}, max {max(tc):.1f}), ratio {mc / mf:.2f}; fused byte model {nbytes / 1e6:.1f} MB = '
      f'{nbytes / mf / 1e6:.2f} TB/s; max |fused - composed| {diff:.3e} at |out|max {scale:.2f}; {windows} windows x {reps} calls', flush=True)  # fmt: skip
