#!/usr/bin/env python3
"""rsa_layernorm at 512 x 512 (180 channels into fp16 hi planes and into bf16 hi + lo planes, 320 channels into fp16 hi planes): device events
around 15 windows of 1000 launches each, after 50 warm-up launches.  RSA_LIB=path times an experiment build (A/B: alternate the two
libraries, one process each, several rounds; profiles/layernorm_forms.txt).  usage: ln_time.py TAG"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from resselt_amd.engine import lib as L  # noqa: E402
from resselt_amd.engine import ops, tensors  # noqa: E402

tag = sys.argv[1]
H = W = 512
dev = torch.device('cuda:0')
lib = L.load()
stream = ops.current_stream_ptr(dev)


def run(C_, form):
    g = torch.Generator(device='cpu').manual_seed(1)
    x = (30.0 + torch.randn((1, (C_ + 3) // 4, H, W, 4), generator=g)).to(dev)
    fmt, lo = (tensors.PF_F16, False) if form == 'f16hi' else (tensors.PF_BF16, True)
    out = tensors.Planes.empty(1, (C_ + 7) // 8, H, W, dev, lo, fmt)
    gm, bt = torch.ones(C_, device=dev), torch.zeros(C_, device=dev)
    lp = L.LayerNormParams()
    lp.batch, lp.H, lp.W, lp.C, lp.eps = 1, H, W, C_, 1e-5
    lp.x_f32, lp.gamma, lp.beta = x.data_ptr(), gm.data_ptr(), bt.data_ptr()
    lp.out_hi, lp.out_lo = out.hi_ptr(), out.lo_ptr()
    lp.out_plane_stride, lp.out_batch_stride, lp.out_fmt = out.plane_stride, out.batch_stride, out.fmt

    def ln():
        assert lib.rsa_layernorm(lp, stream) == 0

    for _ in range(50):
        ln()
    torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(1000):
            ln()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1000 * 1e3)
    ts.sort()
    print(f'TIME {tag} C={C_} {form}: median {statistics.median(ts):.2f} us  min {ts[0]:.2f}  max {ts[-1]:.2f}  (15 windows of 1000 launches)', flush=True)
    assert lib.rsa_check_status() == 0


for cfg in ((180, 'f16hi'), (180, 'bf16hilo'), (320, 'f16hi')):
    run(*cfg)
