"""The cases, the inputs and the float64 reference with its error bound of tests/test_gaterv2_kernels_gpu.py (which derives the bound in
its docstring), in a module of their own because tests/test_gaterv2_capi.py checks the conditioning of the same inputs on the CPU."""

import torch

from resselt_amd.engine import lib_gaterv2 as LG2
from resselt_amd.engine.tensors import PF_BF16, PF_F16

U = 2.0**-24
EPS = 1e-6
FORMATS = [(PF_BF16, True), (PF_BF16, False), (PF_F16, True), (PF_F16, False)]
WIDTHS = [(16, 1), (32, 2), (96, 6), (256, 16), (768, 48), (1024, 64)]  # (C, m)
MAPS = [(1, 1), (2, 3), (127, 1), (8, 16), (3, 43), (15, 20)]  # 1, 6, 127, 128, 129, 300 tokens
CASES = [(c, m, hw) for c, m in WIDTHS for hw in MAPS]


def _fmt_eps(fmt, with_lo):
    e = {(PF_BF16, False): 2.0**-8, (PF_F16, False): 2.0**-11, (PF_BF16, True): 2.0**-16, (PF_F16, True): 2.0**-22}[(fmt, with_lo)]
    return e, (2.0**-25 if fmt == PF_F16 else 0.0)


def make_inputs(c, m, hw, batch=3):
    """[batch, 8 mp | 8 mp | C, H, W]: q and k in their zero-padded planes, v; every |q|, |k| element at least 0.25, one sign per (image, channel)
    shared by q and k."""
    gen = torch.Generator().manual_seed(10000 * m + 100 * hw[0] + hw[1])
    mp8 = (m + 7) // 8 * 8
    x = torch.zeros(batch, 2 * mp8 + c, *hw)
    sign = torch.where(torch.rand(batch, m, 1, 1, generator=gen) < 0.5, 1.0, -1.0)
    for row0 in (0, mp8):
        x[:, row0 : row0 + m] = sign * (0.25 + torch.randn(batch, m, *hw, generator=gen).abs())
    x[:, 2 * mp8 :] = torch.randn(batch, c, *hw, generator=gen)
    if batch > 1:
        x[1, 2 * mp8 :] = x[1, 2 * mp8 :] * 1.7 + 0.6  # other statistics in the second image: a sum leaking across images shows
    return x


def reference(read, c, m, fmt, with_lo):
    """The f64 result and the bound from the f64 values ``read`` [B, 8 mp | 8 mp | C, H, W] the kernel reads; asserts the conditioning."""
    b, _, h, w = read.shape
    n = h * w
    mp8 = (m + 7) // 8 * 8
    q, k, v = read[:, :m].reshape(b, m, n), read[:, mp8 : mp8 + m].reshape(b, m, n), read[:, 2 * mp8 :].reshape(b, c, n)
    assert q.norm(dim=1).min() >= 0.25 and k.norm(dim=1).min() >= 0.25
    qn, kn = q / q.norm(dim=1, keepdim=True), k / k.norm(dim=1, keepdim=True)
    cn = -(-n // LG2.TOKEN_CHUNK)
    rk = (m / 2 + 3) * U
    acc = (128 + cn) * U + rk
    mat, amat = kn @ v.transpose(1, 2), kn.abs() @ v.abs().transpose(1, 2)  # [B, m, C]
    ksum = kn.sum(2) + EPS
    vsum = v.sum(2)
    dM = acc * amat
    dk = acc * kn.abs().sum(2) + U * ksum.abs()
    dv = (128 + cn) * U * v.abs().sum(2)
    den = n + (qn * ksum[:, :, None]).sum(1)  # [B, N]
    assert (den >= n / 2).all()
    dden = (qn.abs() * dk[:, :, None]).sum(1) + (m * U + rk) * (qn * ksum[:, :, None]).abs().sum(1) + U * den.abs()
    t = 1 / den
    rt = dden / den.abs() + U
    num = vsum[:, :, None] + mat.transpose(1, 2) @ qn  # [B, C, N]
    dnum = dv[:, :, None] + dM.transpose(1, 2) @ qn.abs() + (m * U + rk) * (vsum.abs()[:, :, None] + mat.abs().transpose(1, 2) @ qn.abs())
    out = num * t[:, None, :]
    e_fmt, floor = _fmt_eps(fmt, with_lo)
    bar = t.abs()[:, None, :] * dnum + out.abs() * (rt[:, None, :] + U) + e_fmt * out.abs() + floor
    return out.reshape(b, c, h, w), bar.reshape(b, c, h, w)
