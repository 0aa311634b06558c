"""GateR's kernels through the C-ABI against torch on the CPU: the torch-form RMSNorm, the unshuffling relayout (bit-exact), the f32
concatenation and the two passes of the focused linear attention against an f64 formula.

Attention tolerance.  The kernels read the values the planes hold (the f64 formula is given exactly those) and compute in f32: the power
exp2(f log2 t) carries a relative error of about f * |log2 t| * 2^-24 * ln 2 <= 4 * 20 * 4.1e-8 = 3.3e-6, the sums over tokens and channels
add a few f32 roundings, and the result is stored as split planes: hi + lo bf16 keeps 16 bits (2^-17 = 7.6e-6 relative), fp16 hi alone rounds
by up to half an ulp, 2^-11 = 4.9e-4 of the value.  Bound: 2e-5 * |out|max with lo halves, (2^-11 + 2e-5) * |out|max on fp16 hi planes.
First run: 2.6e-6 .. 5.8e-6 relative with lo halves, 4.2e-4 on fp16 hi planes; KV and mean(k) within 3e-7 relative.
Grids: 1x1, 2x3, 3x5, 9x7 and 23x19 -- 437 tokens are four chunks of 128 in the reduction with a last one of 53, and 3 x 5 apply tiles of
8 x 4 with the last column 7 wide and the last row 3 high."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
@pytest.mark.parametrize('C_,hw', [(24, (5, 7)), (48, (17, 31)), (192, (3, 89))])
def test_rmsnorm_torch(device, C_, hw, fmt):
    g = torch.Generator().manual_seed(C_)
    x = torch.randn((2, C_, *hw), generator=g) * 3
    x[1, :, 0, 1] = 0.0  # a pixel of zeros
    w = torch.rand(C_, generator=g) + 0.5
    want = F.rms_norm(x.permute(0, 2, 3, 1).double(), (C_,), w.double(), 1e-6).permute(0, 3, 1, 2)
    xm = nchw_to_f32map(x).to(device)
    out = Planes.empty(2, C_ // 8, *hw, device, True, fmt)
    wd = w.to(device)
    L.check(L.load().rsa_rmsnorm_torch(xm.data_ptr(), 2, hw[0], hw[1], C_, 1e-6, wd.data_ptr(), out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride, fmt,
                                       _stream(device)), 'rsa_rmsnorm_torch')  # fmt: skip
    got = planes_to_nchw(Planes(out.hi.cpu(), out.lo.cpu()), C_).double()
    err = (got - want).abs().max().item()
    print(f'MEASURE rmsnorm_torch C={C_} fmt={fmt}: {err:.3e} (|y|max {want.abs().max():.2f})')
    assert err <= 2e-5 * want.abs().max().item()  # f32 arithmetic + hi/lo planes (16 bits with bf16, 22 with fp16)
    assert torch.equal(got[1, :, 0, 1], torch.zeros(C_, dtype=torch.float64))


def test_rmsnorm_torch_all_zeros(device):
    xm = torch.zeros((1, 6, 4, 5, 4), device=device)
    out = Planes.empty(1, 3, 4, 5, device, True, PF_BF16)
    out.hi.fill_(1.0), out.lo.fill_(1.0)
    w = torch.ones(24, device=device)
    L.check(L.load().rsa_rmsnorm_torch(xm.data_ptr(), 1, 4, 5, 24, 1e-6, w.data_ptr(), out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride, PF_BF16,
                                       _stream(device)), 'rsa_rmsnorm_torch')  # fmt: skip
    assert not out.hi.float().isnan().any() and out.hi.float().abs().max().item() == 0.0 and out.lo.float().abs().max().item() == 0.0


def test_rmsnorm_torch_rejects_bad_arguments(device):
    xm = torch.zeros((1, 6, 4, 5, 4), device=device)
    out = Planes.empty(1, 3, 4, 5, device, True, PF_BF16)
    w = torch.ones(24, device=device)
    lib = L.load()
    assert lib.rsa_rmsnorm_torch(None, 1, 4, 5, 24, 1e-6, w.data_ptr(), out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride, PF_BF16, _stream(device)) == -1
    assert lib.rsa_rmsnorm_torch(xm.data_ptr() + 4, 1, 4, 5, 24, 1e-6, w.data_ptr(), out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride, PF_BF16,
                                 _stream(device)) == -3  # fmt: skip


@pytest.mark.parametrize('cout,hw,n', [(12, (6, 10), 1), (24, (34, 18), 2), (96, (8, 66), 1)])
def test_unshuffle_is_pixel_unshuffle_of_the_convolution_output(device, cout, hw, n):
    """The Downsample path: a 3x3 convolution's ordinary f32 output, then rsa_pixel_unshuffle2 -- bit-exact against torch.pixel_unshuffle."""
    g = torch.Generator().manual_seed(cout)
    cin = 2 * cout
    x = torch.randn((n, cin, *hw), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin**0.5)
    b = torch.randn(cout, generator=g)
    xp = nchw_to_planes(x, True)
    xp = Planes(xp.hi.to(device), xp.lo.to(device))
    wts = ops.ConvWeights.from_oihw(w, b, 3, device=device)
    conv_out = torch.empty((n, cout // 4, *hw, 4), device=device)
    ops.run_convs([ops.conv_params(wts, xp, *hw, out_f32=conv_out)], device)
    out = torch.full((n, cout, hw[0] // 2, hw[1] // 2, 4), float('nan'), device=device)
    L.check(L.load().rsa_pixel_unshuffle2(conv_out.data_ptr(), n, hw[0], hw[1], cout, out.data_ptr(), _stream(device)), 'rsa_pixel_unshuffle2')
    want = F.pixel_unshuffle(f32map_to_nchw(conv_out.cpu(), cout), 2)
    assert torch.equal(f32map_to_nchw(out.cpu(), 4 * cout), want)
    assert (want - F.pixel_unshuffle(F.conv2d(x, w, b, padding=1), 2)).abs().max().item() < 1e-4  # (and the convolution is the convolution)
    lib = L.load()
    assert lib.rsa_pixel_unshuffle2(conv_out.data_ptr(), n, hw[0] - 1, hw[1], cout, out.data_ptr(), _stream(device)) == -1  # odd H
    assert lib.rsa_pixel_unshuffle2(conv_out.data_ptr(), n, hw[0], hw[1], cout, out.data_ptr() + 8, _stream(device)) == -3


def test_f32map_concat(device):
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn((2, 24, 9, 13), generator=g), torch.randn((2, 48, 9, 13), generator=g)
    out = torch.empty((2, 18, 9, 13, 4), device=device)
    ad, bd = a.to(device), nchw_to_f32map(b).to(device)
    L.check(L.load().rsa_f32map_concat(ad.data_ptr(), 24, bd.data_ptr(), 48, 2, 9, 13, out.data_ptr(), _stream(device)), 'rsa_f32map_concat')
    assert torch.equal(f32map_to_nchw(out.cpu(), 72), torch.cat((a, b), 1))


# ------------------------------------------------------------------------------------------------------------------ focused linear attention
def _fla_reference(q, k, v, scale, factor, dw, db, hw):
    """f64, whole tokens [B, N, C]."""
    B, N, C_ = q.shape
    d = C_ // 8

    def focus(t):
        t = (t.clamp(min=0) + 1e-6) / F.softplus(scale)
        n0 = t.norm(dim=-1, keepdim=True)
        t = t**factor
        return t / t.norm(dim=-1, keepdim=True) * n0

    q, k = focus(q), focus(k)
    qh, kh, vh = (t.reshape(B, N, 8, d).transpose(1, 2) for t in (q, k, v))
    kmean = kh.mean(dim=2, keepdim=True)
    kv = kh.transpose(-2, -1) @ vh / N
    z = 1.0 / ((qh * kmean).sum(-1, keepdim=True) + 1e-6)
    out = (qh @ kv * z).transpose(1, 2).reshape(B, N, C_)
    vm = v.transpose(1, 2).reshape(B, C_, *hw)
    conv = F.conv2d(vm, dw.repeat(8, 1, 1, 1), db.repeat(8), padding=2, groups=C_)  # channel c uses filter c % d
    return out + conv.flatten(2).transpose(1, 2), kv, kmean


def _fla_run(device, d, n, hw, fmt, with_lo, seed):
    C_ = 8 * d
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((n, 3 * C_, *hw), generator=g)
    scale, factor = torch.randn(C_, generator=g) * 0.5, 2.0 + 2.0 * torch.rand(C_, generator=g)
    dw, db = torch.randn((d, 1, 5, 5), generator=g) / 5, torch.randn(d, generator=g) * 0.1
    pl = nchw_to_planes(qkv, with_lo, fmt)
    held = planes_to_nchw(pl, 3 * C_).double()  # the values the kernels read
    tok = lambda t: t.flatten(2).transpose(1, 2)  # noqa: E731
    want, kv, kmean = _fla_reference(tok(held[:, :C_]), tok(held[:, C_ : 2 * C_]), tok(held[:, 2 * C_ :]), scale.double(), factor.double(), dw.double(), db.double(), hw)
    pl = Planes(pl.hi.to(device), pl.lo.to(device) if with_lo else None)
    out = Planes.empty(n, C_ // 8, *hw, device, with_lo, fmt)
    lib = L.load()
    nbytes = int(lib.rsa_fla_workspace_bytes(n, hw[0] * hw[1], d))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.zeros(nbytes // 4, device=device)
    sd_, fd, wd, bd = scale.to(device), factor.to(device), dw.reshape(d, 25).contiguous().to(device), db.to(device)
    common = (pl.hi_ptr(), pl.lo_ptr(), pl.plane_stride, pl.batch_stride, n, hw[0], hw[1], d, fmt, sd_.data_ptr(), fd.data_ptr(), ws.data_ptr(), nbytes)
    L.check(lib.rsa_fla_reduce(*common, _stream(device)), 'rsa_fla_reduce')
    torch.cuda.synchronize()
    rec = 8 * d * d + 8 * d
    first = ws[: n * rec].clone()
    L.check(lib.rsa_fla_apply(*common, wd.data_ptr(), bd.data_ptr(), out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride, _stream(device)), 'rsa_fla_apply')
    torch.cuda.synchronize()
    got = planes_to_nchw(Planes(out.hi.cpu(), out.lo.cpu() if with_lo else None), C_).double()
    # a second reduction into a workspace full of NaNs: the same bits
    ws.fill_(float('nan'))
    L.check(lib.rsa_fla_reduce(*common, _stream(device)), 'rsa_fla_reduce')
    torch.cuda.synchronize()
    assert torch.equal(ws[: n * rec].view(torch.int32), first.view(torch.int32))
    fin = first.cpu().double().reshape(n, rec)
    return got, want.transpose(1, 2).reshape(n, C_, *hw), fin[:, : 8 * d * d].reshape(n, 8, d, d), kv, fin[:, 8 * d * d :].reshape(n, 8, 1, d), kmean


@pytest.mark.parametrize('d,n,hw', [(24, 1, (1, 1)), (24, 2, (2, 3)), (24, 1, (3, 5)), (48, 1, (9, 7)), (48, 2, (2, 3)), (24, 1, (23, 19)), (48, 2, (23, 19))])
def test_focused_linear_attention(device, d, n, hw):
    got, want, kv, kv_want, km, km_want = _fla_run(device, d, n, hw, PF_BF16, True, 100 + d + hw[0])
    scale = want.abs().max().item()
    e_kv, e_km, err = (kv - kv_want).abs().max().item(), (km - km_want).abs().max().item(), (got - want).abs().max().item()
    print(f'MEASURE fla d={d} n={n} grid={hw}: out {err:.3e} (|out|max {scale:.2f}), KV {e_kv:.3e} (max {kv_want.abs().max():.2f}), kmean {e_km:.3e}')
    assert e_kv <= 1e-5 * max(1.0, kv_want.abs().max().item()) and e_km <= 1e-5 * max(1.0, km_want.abs().max().item())
    assert err <= 2e-5 * scale


def test_focused_linear_attention_fp16_hi_planes(device):
    got, want, *_ = _fla_run(device, 24, 1, (9, 7), PF_F16, False, 7)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'MEASURE fla fp16 hi planes: out {err:.3e} (|out|max {scale:.2f})')
    assert err <= (2.0**-11 + 2e-5) * scale


def test_fla_rejects_bad_arguments(device):
    lib = L.load()
    pl = Planes.empty(1, 72, 2, 3, device, True, PF_BF16)
    out = Planes.empty(1, 24, 2, 3, device, True, PF_BF16)
    v = torch.ones(192, device=device)
    ws = torch.zeros(int(lib.rsa_fla_workspace_bytes(1, 6, 24)) // 4, device=device)
    args = lambda d=24, hi=pl.hi_ptr(), nbytes=ws.numel() * 4: (hi, pl.lo_ptr(), pl.plane_stride, pl.batch_stride, 1, 2, 3, d, PF_BF16, v.data_ptr(), v.data_ptr(),  # noqa: E731
                                                                  ws.data_ptr(), nbytes)  # fmt: skip
    assert lib.rsa_fla_reduce(*args(d=32), _stream(device)) == -2  # head dimension not compiled
    assert lib.rsa_fla_reduce(*args(nbytes=64), _stream(device)) == -1  # workspace too small
    assert lib.rsa_fla_reduce(*args(hi=pl.hi_ptr() + 8), _stream(device)) == -3  # misaligned planes
    assert lib.rsa_fla_apply(*args(), v.data_ptr(), v.data_ptr(), None, out.lo_ptr(), out.plane_stride, out.batch_stride, _stream(device)) == -1
    assert b'fla_' in lib.rsa_last_error_string()
    assert lib.rsa_fla_workspace_bytes(0, 6, 24) == 0
