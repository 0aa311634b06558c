#!/usr/bin/env python3
"""A/B of the FourierUnit's spectral stage on one spectral grid (default 520 x 261, a little above the 516 x 259 of a 512 x 512 frame padded to
516 x 516) at C2 = 12 and 32 spectral channels:

  A  rsa_gfisr_ln_spectral                         one launch, f32 map -> f32 map (GFISR v1)
  B  rsa_gfisr_spectral + 1x1 rsa_conv2d + GELU    two launches through bf16 split planes with lo halves (GFISRv2's pair; its norm is an
                                                   RMSNorm, the traffic is the same)

Each variant works on SETS rotating buffer sets whose total passes the 256 MB of last-level cache, so a launch reads its input from HBM;
the two variants are timed in alternating rounds of ``reps`` launches between one pair of events, and the median round is reported.
usage: gfisr_spectral_ab.py [H W] [rounds] [reps]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from resselt_amd.engine import lib as L  # noqa: E402
from resselt_amd.engine import lib_gfisr as LG  # noqa: E402
from resselt_amd.engine import lib_gfisr1 as LG1  # noqa: E402
from resselt_amd.engine import ops  # noqa: E402
from resselt_amd.engine.tensors import PF_BF16, Planes  # noqa: E402

a = sys.argv[1:]
H, W = (int(a[0]), int(a[1])) if len(a) > 1 else (520, 261)
rounds = int(a[2]) if len(a) > 2 else 15
reps = int(a[3]) if len(a) > 3 else 32
dev = torch.device('cuda:0')
L.load()
stream = ops.current_stream_ptr(dev)
gen = torch.Generator().manual_seed(0)


def timed(fns):
    """Median over ``rounds`` of the time per launch group, the variants in alternating rounds."""
    for f in fns:
        for i in range(4):
            f(i)
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                f(i)
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return [(statistics.median(v), min(v), max(v)) for v in t]


for C2 in (12, 32):
    p4, pl = (C2 + 3) // 4, (C2 + 7) // 8
    per_set = H * W * (2 * p4 * 16 + pl * 32)
    SETS = max(4, -(-320 * 2**20 // per_set))
    xs = [torch.randn(1, p4, H, W, 4, generator=gen).to(dev) for _ in range(SETS)]
    outs = [torch.empty(1, p4, H, W, 4, device=dev) for _ in range(SETS)]
    sps = [Planes.empty(1, pl, H, W, dev, True, PF_BF16) for _ in range(SETS)]
    vec = lambda n: (torch.randn(n, generator=gen) * 0.3).to(dev)  # noqa: E731
    ln_w, ln_b, fpe_b, fdc_b = 1.0 + vec(8 * pl), vec(8 * pl), vec(8 * pl), vec(8 * pl)
    fpe_w = (torch.randn(8 * pl, 9, generator=gen) / 3.0).to(dev)
    fdc_w = (torch.randn(C2, C2, generator=gen) / C2**0.5).to(dev)
    fused, specs, convs = [], [], []
    cw = ops.ConvWeights.from_oihw(fdc_w.reshape(C2, C2, 1, 1), fdc_b[:C2].contiguous(), 3, fmt=PF_BF16, device=dev)
    for i in range(SETS):
        p = LG1.GfisrLnSpectralParams()
        p.batch, p.H, p.W, p.C, p.eps = 1, H, W, C2, 1e-6
        p.x, p.out = xs[i].data_ptr(), outs[i].data_ptr()
        p.ln_w, p.ln_b, p.fpe_w, p.fpe_b, p.fdc_w, p.fdc_b = (t.data_ptr() for t in (ln_w, ln_b, fpe_w, fpe_b, fdc_w, fdc_b))
        fused.append(p)
        s = LG.GfisrSpectralParams()
        s.batch, s.H, s.W, s.C, s.eps = 1, H, W, C2, 1e-6
        s.x, s.scale, s.offset, s.weight, s.bias = (t.data_ptr() for t in (xs[i], ln_w, ln_b, fpe_w, fpe_b))
        sps[i].bind(s, 'out')
        specs.append(s)
        convs.append(ops.conv_params(cw, sps[i], H, W, act=L.ACT_GELU, out_f32=outs[i]))

    def run_a(i):
        L.launch('rsa_gfisr_ln_spectral', fused[i % SETS], stream)

    def run_b(i):
        L.launch('rsa_gfisr_spectral', specs[i % SETS], stream)
        L.launch('rsa_conv2d', convs[i % SETS], stream)

    def run_b1(i):
        L.launch('rsa_gfisr_spectral', specs[i % SETS], stream)

    (ta, tb, tb1) = timed([run_a, run_b, run_b1])
    px = H * W
    model_a, model_b = px * 2 * C2 * 4, px * (C2 * 4 + 2 * pl * 32 + C2 * 4)
    print(f'{H}x{W} C2 {C2} ({SETS} rotating buffer sets, {rounds} rounds of {reps}):', flush=True)
    print(f'  A fused rsa_gfisr_ln_spectral        {ta[0]:8.1f} us (min {ta[1]:.1f}, max {ta[2]:.1f})  byte model {model_a / px:.0f} B/pixel -> {model_a / ta[0] / 1e6:.2f} TB/s', flush=True)
    print(f'  B rsa_gfisr_spectral + 1x1 GELU conv {tb[0]:8.1f} us (min {tb[1]:.1f}, max {tb[2]:.1f})  byte model {model_b / px:.0f} B/pixel -> {model_b / tb[0] / 1e6:.2f} TB/s'
          f'   (rsa_gfisr_spectral alone {tb1[0]:.1f} us)', flush=True)  # fmt: skip
    print(f'  A / B = {ta[0] / tb[0]:.3f}', flush=True)
    del xs, outs, sps, fused, specs, convs
    torch.cuda.empty_cache()
