"""Kernel-level GPU tests of csrc/plksr.hip: rsa_plk_conv against F.conv2d, GroupNorm statistics / apply against torch, the EA gate."""

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops, plk
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        L.check_status('end of test')


def _stream(device):
    return ops.current_stream_ptr(device)


def _to_map(x):  # [N, C, H, W] -> f32 [N, C/4, H, W, 4]
    n, c, h, w = x.shape
    return x.float().reshape(n, c // 4, 4, h, w).permute(0, 1, 3, 4, 2).contiguous()


def _from_map(m):
    n, p4, h, w, _ = m.shape
    return m.permute(0, 1, 4, 2, 3).reshape(n, 4 * p4, h, w)


MODES = {'bf16x3': (3, PF_BF16), 'fp16': (1, PF_F16)}


def _run_plk(device, n, pdim, k, h, w, mode, seed):
    products, fmt = MODES[mode]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, pdim, h, w, generator=g)
    wt = torch.randn(pdim, pdim, k, k, generator=g) / (pdim * k)
    b = torch.randn(pdim, generator=g)
    xp = Planes.empty(n, pdim // 8, h, w, device, products == 3, fmt)
    ops.nchw_to_planes(x.to(device), xp)
    pp = pdim // 8
    out = Planes.empty(n, 2 * pp + 1, h, w, device, products == 3, fmt)  # PLK writes planes [1, 1 + pp); the others keep a sentinel
    out.hi.fill_(7.0)
    if out.lo is not None:
        out.lo.fill_(0.0)
    blob = plk.pack_plk_weights(wt.to(device), products, fmt)
    bias = plk.plk_bias(b.to(device))
    p = plk.plk_params(blob, bias, k, products, xp, out, 1)
    plk.plk_conv(p, _stream(device))
    got = ops.planes_to_nchw(out, 8 * (2 * pp + 1)).cpu().double()
    x_stored = ops.planes_to_nchw(xp, pdim).cpu().double()
    if mode == 'fp16':
        wref = wt.half().double()
    else:
        wref = wt.double()
    ref = F.conv2d(x_stored, wref, b.double(), padding=k // 2)
    return got, ref, pp


@pytest.mark.parametrize('mode', ['bf16x3', 'fp16'])
@pytest.mark.parametrize('k, pdim, shape', [
    (17, 16, (1, 37, 53)), (3, 8, (1, 37, 53)), (31, 24, (1, 37, 53)), (17, 8, (2, 30, 41)), (17, 24, (2, 19, 70)), (31, 16, (1, 45, 20)),
    (17, 16, (2, 300, 517)), (9, 64, (1, 33, 40)),
])  # fmt: skip
def test_plk_conv_matches_conv2d(device, mode, k, pdim, shape):
    n, h, w = shape
    got, ref, pp = _run_plk(device, n, pdim, k, h, w, mode, seed=k * 100 + pdim)
    tol = (1e-5 if mode == 'bf16x3' else 2e-3) * ref.abs().max().item()
    err = (got[:, 8 : 8 + pdim] - ref).abs().max().item()
    print(f'plk k{k} pdim{pdim} {shape} {mode}: max-abs {err:.3e} / tol {tol:.3e}')
    assert err <= tol
    untouched = torch.cat([got[:, :8], got[:, 8 + pdim :]], 1)
    assert torch.all(untouched == 7.0), 'planes outside the PLK range were written'



@pytest.mark.parametrize('mode', ['bf16x3', 'fp16'])
@pytest.mark.parametrize('k', [17, 31])
@pytest.mark.parametrize('h, w', [(5, 7), (1, 40), (40, 1)])
def test_plk_conv_image_smaller_than_kernel(device, mode, k, h, w):
    """H or W below K / 2: most taps of every output pixel fall in the zero padding, the halo is mostly outside the image."""
    got, ref, pp = _run_plk(device, 2, 16, k, h, w, mode, seed=k * 10 + h)
    tol = (1e-5 if mode == 'bf16x3' else 2e-3) * ref.abs().max().item()
    err = (got[:, 8:24] - ref).abs().max().item()
    print(f'plk k{k} {h}x{w} {mode}: max-abs {err:.3e} / tol {tol:.3e}')
    assert err <= tol
    assert torch.all(torch.cat([got[:, :8], got[:, 24:]], 1) == 7.0), 'planes outside the PLK range were written'


def _gn_ref(x, groups, eps=plk.GN_EPS):
    n, c, h, w = x.shape
    xg = x.double().reshape(n, groups, -1)
    mean = xg.mean(-1)
    var = xg.var(-1, unbiased=False)
    return mean, 1.0 / torch.sqrt(var + eps)


@pytest.mark.parametrize('shape, mean, std', [((2, 32, 37, 53), 0.0, 1.0), ((1, 64, 40, 40), 1e3, 1.0), ((1, 24, 300, 517), -5.0, 0.01),
                                              ((1, 64, 1080, 1920), 0.5, 2.0)])  # fmt: skip
def test_group_norm_stats(device, shape, mean, std):
    g = torch.Generator(device=device).manual_seed(3)
    x = (torch.randn(shape, generator=g, device=device) * std + mean).float()
    xm = _to_map(x)
    ws = plk.group_norm_workspace(shape[0], shape[2], shape[3], 4, device)
    stats = torch.empty((shape[0], 4, 2), dtype=torch.float32, device=device)
    plk.group_norm_stats(xm, shape[1], 4, ws, stats, _stream(device))
    rm, rr = _gn_ref(x, 4)
    got = stats.double()
    assert ((got[..., 0] - rm).abs() <= 1e-5 * rm.abs().clamp_min(std)).all(), (got[..., 0], rm)
    assert ((got[..., 1] - rr).abs() <= 1e-5 * rr).all(), (got[..., 1], rr)


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
def test_group_norm_apply_matches_torch(device, fmt):
    g = torch.Generator().manual_seed(4)
    n, c, h, w = 2, 32, 29, 45
    x = torch.randn(n, c, h, w, generator=g) * 3 + 100.0
    skip = torch.randn(n, c, h, w, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    xm, sm = _to_map(x).to(device), _to_map(skip).to(device)
    ws = plk.group_norm_workspace(n, h, w, 4, device)
    stats = torch.empty((n, 4, 2), dtype=torch.float32, device=device)
    out = Planes.empty(n, c // 8, h, w, device, True, fmt)
    out_f32 = torch.empty_like(xm)
    plk.group_norm_stats(xm, c, 4, ws, stats, _stream(device))
    ap = plk.group_norm_apply_params(xm, c, 4, stats, gamma.to(device), beta.to(device), sm, out, out_f32)
    plk.group_norm_apply(ap, _stream(device))
    ref = F.group_norm(x.double(), 4, gamma.double(), beta.double(), eps=plk.GN_EPS) + skip.double()
    tol = 2e-5 * ref.abs().max().item()
    assert (_from_map(out_f32).cpu().double() - ref).abs().max().item() <= tol
    planes_tol = (2e-5 if fmt == PF_BF16 else 1e-6) * ref.abs().max().item()  # hi + lo: ~16 (bf16) / ~22 (fp16) bits
    assert (ops.planes_to_nchw(out, c).cpu().double() - ref).abs().max().item() <= planes_tol + tol


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
def test_ea_gate_matches_sigmoid_product(device, fmt):
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 2, 24, 31, 19
    x, gate = torch.randn(n, c, h, w, generator=g), 4 * torch.randn(n, c, h, w, generator=g)
    xp = Planes.empty(n, c // 8, h, w, device, True, fmt)
    ops.nchw_to_planes(x.to(device), xp)
    out = Planes.empty(n, c // 8, h, w, device, True, fmt)
    gm = _to_map(gate).to(device)
    plk.ea_gate(plk.ea_gate_params(gm, xp, out, c), _stream(device))
    x_stored = ops.planes_to_nchw(xp, c).cpu().double()
    ref = x_stored * torch.sigmoid(gate.double())
    assert (ops.planes_to_nchw(out, c).cpu().double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    # in place (the engine gates the block buffer itself)
    plk.ea_gate(plk.ea_gate_params(gm, xp, xp, c), _stream(device))
    assert (ops.planes_to_nchw(xp, c).cpu().double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
