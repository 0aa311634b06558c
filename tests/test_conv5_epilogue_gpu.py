"""GPU parity of conv5's own epilogue (conv_common.h `epilogue_c5`: the coded residual stream of an RRDBNet trunk, conv_ring.h XRES 4 / 5).

The epilogue requests the res1 codes of all eight steps of a tile in one burst, the second residual some steps ahead, and guards lanes
outside the map by the buffer range check instead of a branch.  The shapes are the smallest at which that can go wrong:

  (1, 16, 32)    one full tile: each of the eight steps carries its own data
  (1, 17, 33)    four tiles, three of them almost entirely outside the map: guarded lanes load nothing, add nothing, store nothing
  (2, 37, 70)    the batch stride of the code planes; ragged edges
  (1, 300, 610)  380 tiles: several workgroups run two tiles back to back (a burst belongs to its own tile; the pinned ring slots rotate)

Reference: the fp64 convolution of the operands as the kernel reads them (fp16 hi planes, fp16-rounded weights) on the CPU, computed once
per shape, plus the residuals as the planes hold them (hi + decoded code).  Tolerances (those of test_residual_stream_with_8bit_lo_halves):
coded output 2^-19 * max|ref| + 2e-5 -- the coding's step is 2^-19 of the value, 2e-5 the summation order of a 1728-term sum of fp16
products; fp16 lo output 2e-5.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops, tensors
from resselt_amd.engine.tensors import PF_F16

pytestmark = pytest.mark.gpu

PF, PG = 8, 4  # planes of the 64 feature channels / of one growth convolution
SHAPES = [(1, 16, 32), (1, 17, 33), (2, 37, 70), (1, 300, 610)]
KERNELS = ['xres4_one_residual', 'xres4_two_residuals', 'xres5_two_residuals']


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _stream(n, h, w, seed):
    """A 64-channel map as the engine stores it (fp16 hi + 8-bit code), with zeros, fp16 subnormals, ties and hi = +-0 with v != 0 in it."""
    v = _rand((n, 64, h, w), seed)
    v[:, :, 0, :8] = torch.tensor([0.0, 1e-7, -3e-6, 6.1e-5, 0.25, -0.5, 0.24999, 1.0001])
    v[:, :, 1, :6] = torch.tensor([1e-9, -1e-9, 2.9e-8, -2.5e-8, 1.0 + 2.0**-11, -3.0 - 2.0**-9])
    hi, code = tensors.lo8_encode(v)
    return hi, code, tensors.lo8_decode(hi, code)


@functools.lru_cache(maxsize=None)
def _case(n, h, w):
    """Inputs and the CPU reference of one shape, shared by the three kernels (never modified)."""
    g = torch.Generator().manual_seed(15)
    xs, r0s = _stream(n, h, w, 5), _stream(n, h, w, 6)
    growth = _rand((n, 128, h, w), 7).half()  # x1 .. x4: hi planes only
    wt = (torch.rand((64, 192, 3, 3), generator=g) * 2 - 1) / (192 * 9) ** 0.5
    b = (torch.rand((64,), generator=g) * 2 - 1) * 0.1
    cat = torch.cat([xs[0].float(), growth.float()], 1)  # what the multiply reads: hi planes
    y = F.conv2d(cat.double(), wt.half().double(), b.double(), padding=1).float()
    one = y * 0.2 + xs[2]
    return xs, r0s, growth, wt, b, one, one * 0.2 + r0s[2]


def _planes(hi_nchw, n, h, w):
    return hi_nchw.reshape(n, -1, 8, h, w).permute(0, 1, 3, 4, 2)


@pytest.mark.parametrize('n,h,w', SHAPES)
@pytest.mark.parametrize('kernel', KERNELS)
def test_conv5_epilogue(device, kernel, n, h, w):
    xs, r0s, growth, wt, b, ref_one, ref_two = _case(n, h, w)
    two = kernel != 'xres4_one_residual'
    out_lo8 = kernel != 'xres5_two_residuals'

    def workspace():
        return tensors.Planes.empty(n, PF + 4 * PG, h, w, device, True, PF_F16, lo_planes=PF).with_lo8(PF)

    def fill(pl, hc):
        pl.hi[:, :PF] = _planes(hc[0], n, h, w).to(device)
        pl.lo8.copy_(_planes(hc[1], n, h, w).to(device))

    ws, r0, out = workspace(), workspace(), workspace()
    fill(ws, xs)
    ws.hi[:, PF:] = _planes(growth, n, h, w).to(device)
    fill(r0, r0s)
    wts = ops.ConvWeights.from_oihw(wt, b, 1, device=device, fmt=PF_F16)
    kw = dict(res2=(r0, 0, 'lo8'), beta=0.2) if two else {}
    p = ops.conv_params(wts, ws, h, w, cin_planes=24, res1=(ws, 0, 'lo8'), alpha=0.2, out=out, out_lo8=out_lo8, **kw)
    name = L.conv_kernel_name(p)
    assert 'XRES' in name and 'epilogue_c5' in name and f'XR2 {int(two)}' in name, name
    ref = ref_two if two else ref_one
    outs = []
    for order in (0, 1):
        out.hi.fill_(-7.0)  # the growth planes of the output workspace are not this layer's: they must come back untouched
        p.tile_order = order
        ops.run_convs([p], device)
        torch.cuda.synchronize()
        assert L.ring_aborts() == 0
        L.check_status('test')
        assert bool((out.hi[:, PF:] == -7.0).all()), 'a store landed outside the layer\'s own planes'
        if out_lo8:
            got = tensors.planes_to_nchw(tensors.Planes(out.hi[:, :PF].contiguous(), None, out.lo8), 64, lo8=True).cpu()
        else:
            got = tensors.planes_to_nchw(tensors.Planes(out.hi[:, :PF].contiguous(), out.lo[:, :PF].contiguous()), 64).cpu()
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    tol = 2.0**-19 * ref.abs().max().item() + 2e-5 if out_lo8 else 2e-5
    err = (outs[0] - ref).abs().max().item()
    print(f'{kernel} {n}x{h}x{w}: max |error| {err:.3e}, bound {tol:.3e}')
    assert err <= tol, err
