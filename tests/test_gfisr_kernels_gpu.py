"""Kernel-level parity of GFISR v1's entry points (csrc/gfisr1.hip): rsa_gfisr_ln_spectral against the fp64 formula and rsa_plane_window
bit for bit against ``F.pad(..., 'reflect')`` and slicing, and every error code.

The bar of rsa_gfisr_ln_spectral is a first-order forward-error bound derived here, per output element, from the operation counts of the
kernel and the magnitudes of the f64 intermediates (u = 2^-24, the unit roundoff of f32; every product-sum is an fma chain, so a chain of k
terms is within k u of the sum of the absolute values of its terms):

  mean      C additions and a product:                |d mean| <= (C + 1) u A,                 A = max_c |x_c| of the pixel
  x - mean  one subtraction, |x_c - mean| <= 2 A:     |d d_c| <= (C + 3) u A =: dd
  var       C fmas and a product, then the d_c's own error (mean |d_c| <= sigma0 = sqrt(var)):
                                                      |d var| <= (C + 2) u var + 2 dd sigma0
  1 / sqrt(var + eps)   an addition, a square root, a division on top of d var / (2 sigma^2), sigma = sqrt(var + eps):
                                                      relative error rr <= (C + 2) u / 2 + dd / sigma + 3 u
  n_c = d_c rstd        one product:                  |d n_c| <= dd / sigma + |n_c| (rr + u)     <- LayerNorm's conditioning: A / sigma
  v_c = n_c w_c + b_c   one fma:                      |d v_c| <= |w_c| |d n_c| + u |v_c|
  u_c = sum_9 k v + fb_c + v_c   nine fmas and two additions, the "10-term depthwise sum" and its bias:
                                                      |d u_c| <= sum_9 |k| |d v| + |d v_c| + 11 u (sum_9 |k v| + |fb_c| + |v_c|)
  a_o = db_o + sum_c W_oc u_c    C fmas from the bias:
                                                      |d a_o| <= sum_c |W_oc| |d u_c| + (C + 1) u (|db_o| + sum_c |W_oc u_c|)
  z = gelu(a) = 0.5 a (1 + erf(a / sqrt 2))   slope <= 1.13; erff within 4 ulp (HIP's documented accuracy) of a value in [-1, 1], the scaled
            argument, the addition and two products:  |d z| <= 1.13 |d a_o| + 4 u |a_o| + 3 u |z|

Nothing in it is fitted to what the kernel returns.  The inputs keep every pixel's channel standard deviation at 0.1 or more (asserted on
the f64 side), so that A / sigma stays of order 10 to 100 and the bound says something.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gfisr1 as LG1
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, f32map_to_nchw, nchw_to_f32map

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
EPS = 1e-6
N = 2
U = 2.0**-24
E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3
LN_CASES = [((1, 1), 2), ((2, 1), 12), ((1, 2), 4), ((8, 5), 12), ((10, 6), 32), ((7, 36), 6), ((33, 9), 16), ((64, 25), 32)]


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _ln_weights(C2, gen):
    return dict(ln_w=1.0 + 0.25 * torch.randn(C2, generator=gen), ln_b=0.2 * torch.randn(C2, generator=gen),
                fpe_w=torch.randn(C2, 9, generator=gen) / 3.0, fpe_b=torch.randn(C2, generator=gen) / 3.0,
                fdc_w=torch.randn(C2, C2, generator=gen) / C2**0.5, fdc_b=0.2 * torch.randn(C2, generator=gen))  # fmt: skip


def _ln_input(hw, C2, gen):
    if C2 == 2:  # two channels: std = |c1 - c0| / 2 >= 0.5
        c0 = torch.randn(N, 1, *hw, generator=gen) * 3.0
        sign = torch.where(torch.rand(N, 1, *hw, generator=gen) < 0.5, -1.0, 1.0)
        return torch.cat([c0, c0 + sign * (1.0 + torch.randn(N, 1, *hw, generator=gen).abs())], 1)
    return torch.randn(N, C2, *hw, generator=gen) * 3.0 + 1.0


def _ln_reference(x, w, halo_is_ln_b=False):
    """The f64 formula and the forward-error bound of the module docstring, per output element."""
    C2 = x.shape[1]
    d64 = {k: v.double() for k, v in w.items()}
    col = lambda t: t[None, :, None, None]  # noqa: E731
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    d = xd - mean
    var = d.pow(2).mean(1, keepdim=True)
    assert (var.sqrt() >= 0.1).all()  # the inputs are chosen so
    sigma = (var + EPS).sqrt()
    n = d / sigma
    v = n * col(d64['ln_w']) + col(d64['ln_b'])
    k = d64['fpe_w'].reshape(C2, 1, 3, 3)
    if halo_is_ln_b:  # what a halo of LayerNorm values of a zero input would give: NOT the reference
        vp = F.pad(v - col(d64['ln_b']), (1, 1, 1, 1)) + col(d64['ln_b'])
        dw = F.conv2d(vp, k, None, groups=C2)
    else:
        dw = F.conv2d(v, k, None, padding=1, groups=C2)
    u = dw + col(d64['fpe_b']) + v
    Wm = d64['fdc_w']
    a = torch.einsum('oc,nchw->nohw', Wm, u) + col(d64['fdc_b'])
    z = F.gelu(a)
    # ---- the bound
    A = xd.abs().amax(1, keepdim=True)
    dd = (C2 + 3) * U * A
    rr = (C2 + 2) * U / 2 + dd / sigma + 3 * U
    dn = dd / sigma + n.abs() * (rr + U)
    dv = col(d64['ln_w']).abs() * dn + U * v.abs()
    du = F.conv2d(dv, k.abs(), None, padding=1, groups=C2) + dv + 11 * U * (F.conv2d(v.abs(), k.abs(), None, padding=1, groups=C2) + col(d64['fpe_b']).abs() + v.abs())
    da = torch.einsum('oc,nchw->nohw', Wm.abs(), du) + (C2 + 1) * U * (col(d64['fdc_b']).abs() + torch.einsum('oc,nchw->nohw', Wm.abs(), u.abs()))
    bar = 1.13 * da + 4 * U * a.abs() + 3 * U * z.abs()
    return z, bar


def _ln_call(device, x_map, C2, hw, w, override=None, out=None):
    H, W = hw
    p4 = (C2 + 3) // 4
    if out is None:
        out = torch.full((N + 2, p4, H, W, 4), SENTINEL, device=device)  # a guard map in front and one behind
    keep = [x_map.to(device).contiguous()] + [w[k].to(device).contiguous() for k in ('ln_w', 'ln_b', 'fpe_w', 'fpe_b', 'fdc_w', 'fdc_b')]
    p = LG1.GfisrLnSpectralParams()
    p.batch, p.H, p.W, p.C, p.eps = N, H, W, C2, EPS
    p.x, p.ln_w, p.ln_b, p.fpe_w, p.fpe_b, p.fdc_w, p.fdc_b = (t.data_ptr() for t in keep)
    p.out = out[1].data_ptr()
    for k, v in (override or {}).items():
        setattr(p, k, v)
    return L.load().rsa_gfisr_ln_spectral(C.byref(p), _stream(device)), out, keep


@pytest.mark.parametrize('hw,C2', LN_CASES, ids=[f'{h}x{w}-c{c}' for (h, w), c in LN_CASES])
def test_ln_spectral(device, hw, C2):
    gen = torch.Generator().manual_seed(1000 * C2 + 7 * hw[0] + hw[1])
    x, w = _ln_input(hw, C2, gen), _ln_weights(C2, gen)
    ref, bar = _ln_reference(x, w)
    m = nchw_to_f32map(x)
    if C2 % 4:
        m[:, -1, :, :, C2 % 4 :] = float('nan')  # unused components: never read
    rc, out, keep = _ln_call(device, m, C2, hw, w)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all()  # the guard maps
    if C2 % 4:
        assert (got[1 : 1 + N, -1, :, :, C2 % 4 :] == SENTINEL).all()  # components past C are not written
    z = f32map_to_nchw(got[1 : 1 + N], C2).double()
    assert torch.isfinite(z).all()
    err = (z - ref).abs()
    print(f'MEASURE ln_spectral {hw[0]}x{hw[1]} C {C2}: worst error {err.max().item():.3e}, worst error / bar {(err / bar).max().item():.3f}, '
          f'smallest bar {bar.min().item():.2e}, largest {bar.max().item():.2e} (|z|max {ref.abs().max().item():.2f})')  # fmt: skip
    assert (err <= bar).all()
    assert torch.equal(keep[0].cpu().nan_to_num(7.0), m.nan_to_num(7.0))  # the input is left alone


def test_ln_spectral_pads_the_normalised_map_with_zeros(device):
    """The same channel vector at every pixel and ln_b != 0: the interior is one value per channel, and the border shows whether the
    halo holds zeros (the reference: fpe pads the normalised map) or ln_b (a LayerNorm of a zero halo)."""
    hw, C2 = (6, 7), 12
    gen = torch.Generator().manual_seed(5)
    w = _ln_weights(C2, gen)
    w['ln_b'] = 0.5 + torch.rand(C2, generator=gen)
    x = (torch.randn(1, C2, 1, 1, generator=gen) * 3.0 + 1.0).expand(N, C2, *hw).contiguous()
    ref, bar = _ln_reference(x, w)
    other, _ = _ln_reference(x, w, halo_is_ln_b=True)
    rc, out, _ = _ln_call(device, nchw_to_f32map(x), C2, hw, w)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    z = f32map_to_nchw(out.cpu()[1 : 1 + N], C2).double()
    assert ((z - ref).abs() <= bar).all()
    border = torch.ones(hw, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert ((other - ref).abs()[..., border] > 100 * bar[..., border]).any()  # the two differ at the border by far more than the bar
    assert ((other - ref).abs()[..., ~border] <= bar[..., ~border]).all() and ((z - other).abs()[..., border] > bar[..., border]).any()


def test_ln_spectral_error_codes(device):
    hw, C2 = (5, 4), 12
    gen = torch.Generator().manual_seed(1)
    x, w = _ln_input(hw, C2, gen), _ln_weights(C2, gen)
    m = nchw_to_f32map(x)
    call = lambda **fields: _ln_call(device, m, C2, hw, w, override=fields)[0]  # noqa: E731
    assert call() == 0
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(C=0), dict(eps=0.0), dict(reserved0=1), dict(x=None), dict(ln_w=None), dict(ln_b=None),
               dict(fpe_w=None), dict(fpe_b=None), dict(fdc_w=None), dict(fdc_b=None), dict(out=None)):  # fmt: skip
        assert call(**kw) == E_ARG, kw
    for c in (1, 3, 11, 33, 34):
        assert call(C=c) == E_UNSUPPORTED, c
    odd = torch.zeros(64, device=device).data_ptr() + 4
    for key in ('x', 'ln_w', 'ln_b', 'fpe_w', 'fpe_b', 'fdc_w', 'fdc_b', 'out'):
        assert call(**{key: odd}) == E_ALIGN, key
    xm = m.to(device)
    assert call(x=xm.data_ptr(), out=xm.data_ptr()) == E_ARG  # in place: a pixel reads its neighbours
    assert L.load().rsa_gfisr_ln_spectral(None, None) == E_ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- rsa_plane_window
WINDOW_SIZES = [(4, 4), (5, 7), (4, 5), (33, 70)]
WINDOW_FORMS = [(pl, lo, fmt) for pl in (1, 2) for lo in (False, True) for fmt in (PF_BF16, PF_F16)]


def _bits(shape, gen, device):
    """Random 16-bit patterns as int16 (the kernel moves 16-byte units: the plane format does not matter to it)."""
    return torch.randint(-32768, 32767, shape, generator=gen, dtype=torch.int16).to(device)


class _Guarded:
    """``planes`` planes of [h][w][8] 16-bit values at plane 1 of a sentinel-filled buffer whose plane stride is 5 units larger than the map."""

    def __init__(self, planes, h, w, device, fmt, with_lo, content=None):
        self.planes, self.h, self.w, self.stride = planes, h, w, h * w + 5
        dt = torch.float16 if fmt == PF_F16 else torch.bfloat16
        mk = lambda: torch.full((N, planes + 2, self.stride, 8), SENTINEL, dtype=dt, device=device)  # noqa: E731
        self.hi, self.lo = mk(), (mk() if with_lo else None)
        if content is not None:
            for t, c in zip((self.hi, self.lo), content):
                if t is not None:
                    t.view(torch.int16)[:, 1 : 1 + planes, : h * w] = c.reshape(N, planes, h * w, 8)

    def bind(self, p, prefix):
        setattr(p, f'{prefix}_hi', self.hi[:, 1].data_ptr())
        setattr(p, f'{prefix}_lo', None if self.lo is None else self.lo[:, 1].data_ptr())
        setattr(p, f'{prefix}_plane_stride', self.stride)
        setattr(p, f'{prefix}_batch_stride', (self.planes + 2) * self.stride)

    def payload(self, t):
        return t.view(torch.int16)[:, 1 : 1 + self.planes, : self.h * self.w].reshape(N, self.planes, self.h, self.w, 8).cpu()

    def guards_untouched(self):
        for t in (self.hi, self.lo) if self.lo is not None else (self.hi,):
            assert (t[:, 0] == SENTINEL).all() and (t[:, -1] == SENTINEL).all() and (t[:, 1:-1, self.h * self.w :] == SENTINEL).all()


def _window(device, src: _Guarded, dst: _Guarded, top, left, override=None):
    p = LG1.PlaneWindowParams()
    p.batch, p.planes, p.H, p.W, p.out_H, p.out_W, p.top, p.left = N, src.planes, src.h, src.w, dst.h, dst.w, top, left
    src.bind(p, 'in')
    dst.bind(p, 'out')
    for k, v in (override or {}).items():
        setattr(p, k, v)
    return L.load().rsa_plane_window(C.byref(p), _stream(device))


def _reflect_pad(c, H, W):
    """[N, P, H, W, 8] int16 -> torch's reflect pad (2, 2 + W % 2, 2, 2 + H % 2) of every channel, exactly (16-bit integers in float64)."""
    t = c.cpu().double().permute(0, 1, 4, 2, 3).reshape(N, -1, H, W)
    t = F.pad(t, (2, 2 + W % 2, 2, 2 + H % 2), mode='reflect')
    return t.reshape(N, c.shape[1], 8, *t.shape[-2:]).permute(0, 1, 3, 4, 2).to(torch.int16)


@pytest.mark.parametrize('planes,with_lo,fmt', WINDOW_FORMS, ids=[f'p{pl}-{"lo" if lo else "hi"}-{"f16" if f else "bf16"}' for pl, lo, f in WINDOW_FORMS])
@pytest.mark.parametrize('hw', WINDOW_SIZES, ids=[f'{h}x{w}' for h, w in WINDOW_SIZES])
def test_plane_window_pad_and_crop(device, hw, planes, with_lo, fmt):
    H, W = hw
    Hp, Wp = H + 4 + H % 2, W + 4 + W % 2
    gen = torch.Generator().manual_seed(100 * H + W + planes)
    content = (_bits((N, planes, H, W, 8), gen, device), _bits((N, planes, H, W, 8), gen, device))
    src = _Guarded(planes, H, W, device, fmt, with_lo, content)
    pad = _Guarded(planes, Hp, Wp, device, fmt, with_lo)
    assert _window(device, src, pad, 2, 2) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    for t, c in zip((pad.hi, pad.lo), content):
        if t is not None:
            assert torch.equal(pad.payload(t), _reflect_pad(c, H, W))  # bit for bit
    pad.guards_untouched()
    back = _Guarded(planes, H, W, device, fmt, with_lo)
    assert _window(device, pad, back, -2, -2) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    for t, u, c in zip((back.hi, back.lo), (pad.hi, pad.lo), content):
        if t is not None:
            assert torch.equal(back.payload(t), pad.payload(u)[:, :, 2 : 2 + H, 2 : 2 + W])  # the crop is a slice
            assert torch.equal(back.payload(t), c.cpu())  # and the exact inverse of the pad on the interior
    back.guards_untouched()
    src.guards_untouched()


def test_plane_window_error_codes(device):
    H, W = 4, 5
    gen = torch.Generator().manual_seed(3)
    content = (_bits((N, 1, H, W, 8), gen, device), _bits((N, 1, H, W, 8), gen, device))
    src = _Guarded(1, H, W, device, PF_BF16, True, content)
    dst = _Guarded(1, 8, 10, device, PF_BF16, True)
    call = lambda top=2, left=2, **fields: _window(device, src, dst, top, left, override=fields)  # noqa: E731
    assert call() == 0
    for kw in (dict(batch=0), dict(planes=0), dict(H=0), dict(W=0), dict(out_H=0), dict(out_W=0), dict(in_hi=None), dict(out_hi=None), dict(in_lo=None),
               dict(out_lo=None), dict(in_plane_stride=H * W - 1), dict(out_plane_stride=79)):  # fmt: skip
        assert call(**kw) == E_ARG, kw
    # a pad >= the side needs a second reflection: refused, as torch refuses it
    assert call(top=4) == E_ARG and call(left=5) == E_ARG and call(top=3) == 0 and call(left=4) == 0
    # ... and so does one at the far side (the stride is only a number here: the call is refused before anything is launched)
    assert call(out_H=2 + 2 * (H - 1) + 2, out_plane_stride=400) == E_ARG and call(out_W=2 + 2 * (W - 1) + 2, out_plane_stride=400) == E_ARG
    assert call(H=2) == E_ARG
    odd = torch.zeros(64, device=device).data_ptr() + 8
    for key in ('in_hi', 'in_lo', 'out_hi', 'out_lo'):
        assert call(**{key: odd}) == E_ALIGN, key
    assert L.load().rsa_plane_window(None, None) == E_ARG
    torch.cuda.synchronize()
    dst.guards_untouched()
