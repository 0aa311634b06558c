"""GPU checks of the two pieces RCAN adds to the library: channel pooling in the convolution epilogue (``rsa_conv_params.pool_sums``) and
``rsa_rcab_tail``.

Pooling.  The planes (and the f32 map) of a pooled launch are the bits of the same launch without pooling; two runs give the same sums; and
the sums, added over the slots in f64, equal the f64 sum of the launch's own ``out_f32`` within  d * 2^-24 * sum|v|  with d = 11: the depth
of the kernel's reduction tree (conv_common.h, EM 5: seven additions in the lane, four butterfly steps over the 16 lanes of a row) -- the
first-order bound of a summation tree of that depth in f32; the slot sum itself is in f64.
Tail.  The gate against an f64 computation from the same sums within 4 * 2^-24 (the final rounding to f32 and the f64 -> f32 of the
operands of the reference leave nothing more: a sigmoid is at most 1 and has slope <= 1/4); the output planes against
``x + gate * y`` of the dequantised operands within one unit of the written format (2^-8 relative for bf16 hi alone, 2^-11 for fp16 hi alone,
2^-16 / 2^-21 with lo halves; fp16 halves cannot step finer than the format's subnormal spacing 2^-24, which is added).
"""

import ctypes as C

import pytest
import torch

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops, tensors
from resselt_amd.engine.tensors import PF_BF16, PF_F16

pytestmark = pytest.mark.gpu

DEPTH = 11  # conv_common.h, EM 5


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _setup(device, n, c, h, w, fmt, products, seed):
    x = _rand((n, c, h, w), seed, 4.0)
    wt = _rand((c, c, 3, 3), seed + 1, 1.0 / (c * 9) ** 0.5)
    b = _rand((c,), seed + 2, 0.5)
    wts = ops.ConvWeights.from_oihw(wt, b, products, device=device, fmt=fmt)
    xin = tensors.nchw_to_planes(x.to(device), with_lo=products == 3, fmt=fmt)
    return wts, xin


@pytest.mark.parametrize('fmt,products', [(PF_BF16, 3), (PF_F16, 1)])
@pytest.mark.parametrize('n,c,h,w', [(1, 64, 37, 53), (2, 64, 9, 130), (2, 48, 37, 53), (1, 48, 9, 130), (1, 64, 64, 96)])
def test_pooled_convolution(device, n, c, h, w, fmt, products):
    wts, xin = _setup(device, n, c, h, w, fmt, products, 11 * c + h)
    with_lo = products == 3

    def run(pool: bool):
        out = tensors.Planes.empty(n, c // 8, h, w, device, with_lo=with_lo, fmt=fmt)
        of32 = tensors.empty_f32map(n, c, h, w, device)
        p = ops.conv_params(wts, xin, h, w, out=out, out_f32=of32)
        sums = None
        if pool:
            slots = ops.conv_pool_slots(p)
            assert slots == -(-h // 16) * -(-w // 32) * (8 if c == 48 else 4)
            sums = torch.full((n, slots, c), float('nan'), dtype=torch.float32, device=device)
            p = ops.conv_params(wts, xin, h, w, out=out, out_f32=of32, pool_sums=sums)
            assert 'XRES 7' in L.conv_kernel_name(p)
        ops.run_convs([p], device)
        torch.cuda.synchronize()
        assert L.ring_aborts() == 0
        L.check_status('test')
        return out, of32, sums

    plain, plain32, _ = run(False)
    pooled, pooled32, sums = run(True)
    again, _, sums2 = run(True)
    assert torch.equal(plain.hi, pooled.hi) and torch.equal(plain32, pooled32)
    if with_lo:
        assert torch.equal(plain.lo, pooled.lo)
    assert torch.equal(sums, sums2) and torch.equal(again.hi, pooled.hi)  # a fixed reduction order: run to run, bit for bit
    assert bool(torch.isfinite(sums).all())  # every slot entry was written
    v = tensors.f32map_to_nchw(pooled32, c).double()
    want = v.sum(dim=(2, 3))
    got = sums.double().sum(dim=1)
    bound = DEPTH * 2.0**-24 * v.abs().sum(dim=(2, 3))
    err = (got - want).abs()
    print(f'pool {n}x{c}x{h}x{w} fmt {fmt}: max err / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())


def test_pooling_unsupported_forms(device):
    n, h, w = 1, 20, 40
    lib = L.load()
    # 32 output channels (the two-stream shape), a residual, a final store, one bf16 product: not compiled
    wts32, xin32 = _setup(device, n, 32, h, w, PF_BF16, 3, 5)
    wts64, xin64 = _setup(device, n, 64, h, w, PF_BF16, 3, 6)
    wts64p1, xin64p1 = _setup(device, n, 64, h, w, PF_BF16, 1, 7)
    out32 = tensors.Planes.empty(n, 4, h, w, device)
    out64 = tensors.Planes.empty(n, 8, h, w, device)
    res = tensors.empty_f32map(n, 64, h, w, device)
    nchw = torch.empty((n, 64, h, w), dtype=torch.float32, device=device)
    sums = torch.zeros((n, 64, 64), dtype=torch.float32, device=device)
    cases = [
        ops.conv_params(wts32, xin32, h, w, out=out32),
        ops.conv_params(wts64, xin64, h, w, out=out64, res1=res),
        ops.conv_params(wts64, xin64, h, w, out_nchw=nchw),
        ops.conv_params(wts64, xin64, h, w, out=out64, act=L.ACT_GELU),
        ops.conv_params(wts64p1, xin64p1, h, w, out=tensors.Planes.empty(n, 8, h, w, device, with_lo=False)),
    ]
    for p in cases:
        assert ops.conv_pool_slots(p) is None
        p.pool_sums = sums.data_ptr()
        assert lib.rsa_conv2d(C.byref(p), C.c_void_p(ops.current_stream_ptr(device))) == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(sums.abs().max()) == 0.0  # nothing was launched


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
@pytest.mark.parametrize('with_lo', [True, False])
@pytest.mark.parametrize('n,c,h,w,hidden,slots', [(2, 64, 37, 53, 4, 24), (1, 48, 9, 130, 6, 40), (1, 64, 5, 7, 4, 1037)])
def test_rcab_tail(device, n, c, h, w, hidden, slots, with_lo, fmt):
    lib = L.load()
    cp = (c + 15) // 16 * 16
    x, y = _rand((n, c, h, w), 1, 100.0), _rand((n, c, h, w), 2, 30.0)
    sums = _rand((n, slots, cp), 3, 50.0) + 2.0
    w1, b1 = _rand((hidden, c), 4, 0.3), _rand((hidden,), 5, 0.3)
    w2, b2 = _rand((c, hidden), 6, 1.0), _rand((c,), 7, 0.5)
    xp = tensors.nchw_to_planes(x.to(device), with_lo=with_lo, fmt=fmt)
    yp = tensors.nchw_to_planes(y.to(device), with_lo=with_lo, fmt=fmt)
    out = tensors.Planes.empty(n, c // 8, h, w, device, with_lo=with_lo, fmt=fmt)
    gate = torch.empty((n, c), dtype=torch.float32, device=device)
    dv = [t.to(device).contiguous() for t in (sums, w1, b1, w2, b2)]
    stream = C.c_void_p(ops.current_stream_ptr(device))

    def call(sums_ptr, dst):
        L.check(lib.rsa_rcab_tail(sums_ptr, slots, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), hidden, gate.data_ptr(),
                                  yp.hi_ptr(), yp.lo_ptr(), yp.plane_stride, yp.batch_stride, xp.hi_ptr(), xp.lo_ptr(), xp.plane_stride, xp.batch_stride,
                                  dst.hi_ptr(), dst.lo_ptr(), dst.plane_stride, dst.batch_stride, n, h, w, c, fmt, stream), 'rsa_rcab_tail')  # fmt: skip
        torch.cuda.synchronize()

    call(dv[0].data_ptr(), out)
    mean = sums.double().sum(dim=1)[:, :c] / (h * w)
    hid = torch.relu(mean @ w1.double().T + b1.double())
    want_gate = torch.sigmoid(hid @ w2.double().T + b2.double())
    gerr = (gate.cpu().double() - want_gate).abs().max().item()
    print(f'gate err {gerr:.3e}')
    assert gerr <= 4 * 2.0**-24
    xq, yq = tensors.planes_to_nchw(xp, c).cpu().double(), tensors.planes_to_nchw(yp, c).cpu().double()
    want = xq + gate.cpu().double()[:, :, None, None] * yq
    got = tensors.planes_to_nchw(out, c).cpu().double()
    bits = {(PF_BF16, False): 8, (PF_BF16, True): 16, (PF_F16, False): 11, (PF_F16, True): 21}[(fmt, with_lo)]
    # one unit of the written format at the value: its relative spacing, and for fp16 the absolute spacing 2^-24 of the format's subnormals,
    # below which neither half can resolve (a bf16 half has the exponent range of f32)
    unit = 2.0**-bits * want.abs() + (2.0**-24 if fmt == PF_F16 else 2.0**-60)
    assert bool(((got - want).abs() <= unit).all()), float(((got - want).abs() / unit).max())
    # a gate given from outside (the composed path), written in place over x
    before = gate.clone()
    call(None, xp)
    assert torch.equal(gate, before)
    assert torch.equal(xp.hi, out.hi) and (not with_lo or torch.equal(xp.lo, out.lo))


def test_rcab_tail_argument_checks(device):
    lib = L.load()
    z = torch.zeros(4096, dtype=torch.float32, device=device)
    p = z.data_ptr()

    def call(c=64, hidden=4, slots=4, sums=p, off=0):
        return lib.rsa_rcab_tail(sums, slots, p, p, p, p, hidden, p, p + off, None, 64, 512, p, None, 64, 512, p, None, 64, 512, 1, 8, 8, c, 0, None)

    assert call(c=60) == -1 and call(c=520) == -1 and call(hidden=129) == -1 and call(slots=0) == -1
    assert call(off=8) == -3
