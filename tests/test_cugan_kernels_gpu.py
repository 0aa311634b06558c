"""The Real-CUGAN kernels (csrc/cugan.hip) one by one against torch on windows of larger grids: rsa_deconv (k2 s2 p0, k4 s2 p3, k5 s3 p2)
and rsa_conv_s2 at even and odd origins, both with bias, LeakyReLU and a residual window, in three bf16 products and one fp16 product, on
windows of one workgroup and of many with ragged last tiles; rsa_region_se against the mean of the crop, with a ragged last row chunk and
on a 540 x 960 window; the input and output stages (8-bit stores bit-exact)."""

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import cugan as CG
from resselt_amd.engine import lib as L
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu

PRECISIONS = {'bf16x3': (3, PF_BF16, 2e-5), 'fp16': (1, PF_F16, 2e-3)}  # products, plane format, tolerance relative to max|ref|


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def _planes(x, products, fmt, device):
    p = nchw_to_planes(x.to(device), with_lo=products == 3, fmt=fmt)
    return p, planes_to_nchw(p, x.shape[1]).double()  # the values the kernel reads


def _win(t, w):
    return t[:, :, w.y0 : w.y0 + w.h, w.x0 : w.x0 + w.w]


def _run_resample(device, transposed, k, s, pad, cin, cout, prec, win_in, seed, residual=True):
    products, fmt, tol = PRECISIONS[prec]
    n = 2
    gh, gw = win_in.y0 + win_in.h + 3, win_in.x0 + win_in.w + 2
    x = _rand((n, cin, gh, gw), seed)
    xp, xv = _planes(x, products, fmt, device)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = _rand(wshape, seed + 1, 1.0 / (cin * k * k / (s * s if transposed else 1)) ** 0.5)
    b = _rand((cout,), seed + 2, 0.2)
    wts = CG.ResampleWeights.make(w, b, s, pad, transposed, products, fmt, device)
    if transposed:
        oh, ow = CG.deconv_out(win_in.h, k, s, pad), CG.deconv_out(win_in.w, k, s, pad)
    else:
        oh, ow = win_in.h // 2, win_in.w // 2
    oy0, ox0 = 2, 3
    out = Planes.empty(n, (cout + 7) // 8, oh + 5, ow + 4, device, with_lo=products == 3, fmt=fmt)
    out.hi.zero_()
    if out.lo is not None:
        out.lo.zero_()
    omap = torch.zeros((n, (cout + 3) // 4, oh + 5, ow + 4, 4), dtype=torch.float32, device=device)
    res = rv = None
    ry0, rx0 = 1, 4
    if residual:
        r = _rand((n, cout, oh + 2, ow + 6), seed + 3)
        res, rv = _planes(r, products, fmt, device)
    p = CG.resample_params(wts, xp, win_in, out=out, out_f32=omap, out_y0=oy0, out_x0=ox0, res=res, res_y0=ry0, res_x0=rx0, lrelu=True)
    CG.run_resample(p, transposed, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    xw = _win(xv, win_in).cpu()
    if transposed:
        ref = F.conv_transpose2d(xw, w.double(), b.double(), stride=s, padding=pad)
    else:
        ref = F.conv2d(xw, w.double(), b.double(), stride=2)
    ref = F.leaky_relu(ref, 0.1)
    if residual:
        ref = ref + rv.cpu()[:, :, ry0 : ry0 + oh, rx0 : rx0 + ow]
    got_map = torch.from_numpy(omap.cpu().numpy()).permute(0, 1, 4, 2, 3).reshape(n, -1, oh + 5, ow + 4)[:, :cout].double()
    got_pl = planes_to_nchw(out, cout).double().cpu()
    ow_ = CG.Win(oy0, ox0, oh, ow)
    bar = tol * max(1.0, ref.abs().max().item())
    assert (_win(got_map, ow_) - ref).abs().max().item() <= bar
    assert (_win(got_pl, ow_) - ref).abs().max().item() <= bar + 4e-3 * (products == 1) * ref.abs().max().item()
    # nothing outside the output window is written
    mask = torch.ones_like(got_map, dtype=torch.bool)
    _win(mask, ow_)[:] = False
    assert got_map[mask].abs().max().item() == 0.0 and got_pl[mask].abs().max().item() == 0.0


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('k, s, pad', [(2, 2, 0), (4, 2, 3), (5, 3, 2)])
@pytest.mark.parametrize('cin, cout', [(64, 64), (128, 128), (64, 3), (12, 128), (3, 12)])
def test_deconv_matches_conv_transpose2d(device, k, s, pad, cin, cout, prec):
    _run_resample(device, True, k, s, pad, cin, cout, prec, CG.Win(3, 5, 9, 12), seed=k * 100 + cin + cout)


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('origin', [(2, 4), (3, 5), (1, 2)])
@pytest.mark.parametrize('cin, cout', [(64, 64), (128, 128), (12, 3)])
def test_conv_s2_matches_strided_conv2d(device, origin, cin, cout, prec):
    win = CG.Win(origin[0], origin[1], 15, 18)  # odd height: the last row is dropped (floor), as nn.Conv2d does
    _run_resample(device, False, 2, 2, 0, cin, cout, prec, win, seed=origin[0] + cin + cout, residual=cout != 3)


def test_conv_s2_parity_matters(device):
    """The same window one pixel further gives different pixel pairs: a kernel that paired (2i, 2i+1) of the grid would fail one of them."""
    for y0 in (2, 3):
        _run_resample(device, False, 2, 2, 0, 64, 64, 'bf16x3', CG.Win(y0, y0, 10, 10), seed=7)


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('k, s, pad', [(2, 2, 0), (4, 2, 3), (5, 3, 2)])
@pytest.mark.parametrize('cout', [3, 12, 24, 64, 128])
def test_deconv_many_workgroups_ragged_tiles(device, k, s, pad, cout, prec):
    """A 61 x 83 input window: several workgroups per phase in both directions, ragged last tiles; couts reach every CT instantiation."""
    _run_resample(device, True, k, s, pad, 64, cout, prec, CG.Win(2, 3, 61, 83), seed=k * 1000 + cout)


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('origin', [(2, 4), (3, 5)])
@pytest.mark.parametrize('cout', [3, 12, 24, 64, 128])
def test_conv_s2_many_workgroups_ragged_tiles(device, origin, cout, prec):
    win = CG.Win(origin[0], origin[1], 61, 83)  # odd both ways: the last row and column are dropped
    _run_resample(device, False, 2, 2, 0, 64, cout, prec, win, seed=origin[0] * 1000 + cout, residual=cout != 3)


def _run_region_se(device, C, prec, n, gh, gw, win, seed):
    products, fmt, tol = PRECISIONS[prec]
    x = _rand((n, C, gh, gw), seed) + 0.3
    xp, xv = _planes(x, products, fmt, device)
    hid = C // 8
    w1, b1 = _rand((hid, C, 1, 1), seed + 1, 0.5), _rand((hid,), seed + 2, 0.5)
    w2, b2 = _rand((C, hid, 1, 1), seed + 3, 0.5), _rand((C,), seed + 4, 0.5)
    se = CG.SEWeights.make(w1, b1, w2, b2, device)
    ws = CG.region_se_workspace(n, win.h, xp.planes, device)
    gate = torch.empty((n, C), dtype=torch.float32, device=device)
    CG.run('rsa_region_se', CG.region_se_params(se, xp, win, ws, gate), device=device)
    torch.cuda.synchronize()
    xv = xv.cpu()
    m = _win(xv, win).mean((2, 3), keepdim=True)
    g = torch.sigmoid(F.conv2d(F.relu(F.conv2d(m, w1.double(), b1.double())), w2.double(), b2.double()))
    assert (gate.cpu().double() - g.reshape(n, C)).abs().max().item() <= 1e-6
    ref = xv.clone()
    _win(ref, win).mul_(g)
    got = planes_to_nchw(xp, C).double().cpu()
    assert (got - ref).abs().max().item() <= tol * ref.abs().max().item()
    mask = torch.ones_like(ref, dtype=torch.bool)
    _win(mask, win)[:] = False
    assert torch.equal(got[mask], xv[mask])  # outside the window: untouched


@pytest.mark.parametrize('prec', list(PRECISIONS))
@pytest.mark.parametrize('C', [64, 128])
def test_region_se_matches_torch(device, C, prec):
    _run_region_se(device, C, prec, 2, 37, 45, CG.Win(3, 5, 29, 33), seed=11)


@pytest.mark.parametrize('prec', list(PRECISIONS))
def test_region_se_ragged_last_chunk(device, prec):
    """53 window rows: three full 16-row chunks and a ragged one of 5 rows, whose sums must reach the mean."""
    _run_region_se(device, 128, prec, 2, 60, 41, CG.Win(4, 3, 53, 37), seed=31)


def test_region_se_large_window(device):
    """A 540 x 960 window (the 4x model's input frame) at C = 64: 34 chunks, a ragged last one, the gate still within 1e-6 of float64."""
    _run_region_se(device, 64, 'bf16x3', 1, 545, 966, CG.Win(3, 5, 540, 960), seed=41)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize('pro, unshuffle, pad', [(False, 1, 18), (True, 1, 19), (False, 2, 38)])
def test_input_stage_matches_torch(device, dtype, pro, unshuffle, pad):
    n, c, h, w = 2, 3, 41, 46
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)
    xf = img.permute(0, 3, 1, 2).float() / 255 if dtype == torch.uint8 else torch.rand((n, c, h, w), generator=g).to(dtype)
    xin = img if dtype == torch.uint8 else xf
    ph, pw = h + 1, w + 2
    H, W = (ph + 2 * pad) // unshuffle, (pw + 2 * pad) // unshuffle
    out = Planes.empty(n, (c * unshuffle**2 + 7) // 8, H, W, device, with_lo=True, fmt=PF_BF16)
    sc, sh = (0.7, 0.15) if pro else (1.0, 0.0)
    CG.run('rsa_cugan_input', CG.input_params(xin.to(device), (n, c, h, w), out, pad, pad, unshuffle, sc, sh), device=device)
    torch.cuda.synchronize()
    v = xf.float() * sc + sh if pro else xf.float()
    v = F.pad(v, (pad, unshuffle * W - pad - w, pad, unshuffle * H - pad - h), mode='reflect')
    if unshuffle > 1:
        v = F.pixel_unshuffle(v, unshuffle)
    ref = nchw_to_planes(v, with_lo=True)
    if pro:  # v * 0.7 + 0.15 may be one fused multiply-add on the device; hi + lo keeps ~16 bits of it
        got = planes_to_nchw(out, c * unshuffle**2).cpu()
        assert (got - v).abs().max().item() <= 1e-5
    else:
        assert torch.equal(out.hi.cpu(), ref.hi) and torch.equal(out.lo.cpu(), ref.lo)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize('r, base_div, pro', [(1, 0, False), (2, 4, False), (2, 2, False), (1, 0, True), (2, 4, True)])
def test_output_stage_matches_torch(device, dtype, r, base_div, pro):
    n, C, h0, w0 = 2, 3, 9, 11
    s = base_div if base_div else 2
    oh, ow = h0 * s, w0 * s
    mh, mw = oh // r + 7, ow // r + 5
    y0, x0 = 3, 2
    fm = _rand((n, C * r * r, mh, mw), 21) * 0.6 + 0.5
    fmap = nchw_to_f32map(fm).to(device)
    g = torch.Generator().manual_seed(22)
    img = torch.randint(0, 256, (n, h0, w0, C), generator=g, dtype=torch.uint8)
    base = img if dtype == torch.uint8 else torch.rand((n, C, h0, w0), generator=g).to(dtype)
    out = torch.empty((n, oh, ow, C) if dtype == torch.uint8 else (n, C, oh, ow), dtype=dtype, device=device)
    bs, bsh, osh, odv = (0.7, 0.15, 0.15, 0.7) if pro else (1.0, 0.0, 0.0, 1.0)
    p = CG.output_params(fmap, C, y0, x0, r, out, (oh, ow), base=base.to(device) if base_div else None, base_hw=(h0, w0), base_div=max(base_div, 1),
                         base_scale=bs, base_shift=bsh, out_shift=osh, out_div=odv)  # fmt: skip
    CG.run('rsa_cugan_output', p, device=device)
    torch.cuda.synchronize()
    v = fm[:, :, y0 : y0 + oh // r, x0 : x0 + ow // r]
    v = F.pixel_shuffle(v, r) if r > 1 else v
    if base_div:
        bf = img.permute(0, 3, 1, 2).float() / 255 if dtype == torch.uint8 else base.float()
        v = v + F.interpolate(bf * bs + bsh if pro else bf, scale_factor=base_div, mode='nearest')
    if pro:
        v = (v - 0.15) / 0.7
    got = out.cpu()
    if dtype == torch.uint8:
        ref = (v.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        if pro:  # fused multiply-adds may move a value by an ulp across a rounding boundary
            assert (got.int() - ref.int()).abs().max().item() <= 1
        else:
            assert torch.equal(got, ref)
    elif pro:
        assert (got.float() - v.to(dtype).float()).abs().max().item() <= (1e-6 if dtype == torch.float32 else 1e-2)
    else:
        assert torch.equal(got, v.to(dtype))


def test_argument_validation(device):
    lib = L.load()
    import ctypes

    p = L.ResampleConvParams()
    assert lib.rsa_deconv(ctypes.byref(p), None) == -1
    p.batch, p.cin_planes, p.cout, p.in_W, p.ksize, p.stride, p.pad = 1, 8, 64, 16, 7, 2, 0
    assert lib.rsa_deconv(ctypes.byref(p), None) == -2  # ksize 7
    p.ksize = 3
    assert lib.rsa_conv_s2(ctypes.byref(p), None) == -2  # conv_s2 is k2 s2 p0 only
    assert lib.rsa_region_se(None, None) == -1
    assert lib.rsa_cugan_input(None, None) == -1 and lib.rsa_cugan_output(None, None) == -1
