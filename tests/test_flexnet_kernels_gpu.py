"""FlexNet's kernels through the C-ABI against f64 formulas that are given exactly the values the planes and maps hold.

Bounds (derived, not measured; every case prints a MEASURE line).  u = 2^-24 is one f32 rounding relative to the sum it belongs to; a value
stored as split planes keeps 16 bits with bf16 hi + lo (2^-17 relative), 11 with fp16 hi alone (2^-11), 8 with bf16 hi alone (2^-8).

norm_shift.  1 / rms carries the C squares and their sum, the mean, + eps, sqrt and the division: at most (C / 2 + 3) u relative (a sum of
positive terms); the normalised value two more products; the 25 taps 25 u relative to S = sum |w y|.  Bound per output:
(C / 2 + 30) u S + fmt |out|, S taken as its maximum over the map.
window_attn.  The f64 formula reads hi + lo (three products) or hi alone (one product), so what remains is: the lo lo term the three-product
form drops (|lo| <= 2^-9 |hi|: 2^-18 relative to L = sum_c |q_c k_c|) and the f32 accumulation of 3 C (or C) exact products: d = (2^-18 + 3 C u) L
per logit with three products, C u L with one.  A softmax weight moves by 2 d relatively (numerator and sum); expf and the subtraction of
the maximum add < 4e-6 where the weight is not negligible (|logit - max| < 40); the weights enter the second product as hi + lo (2^-18
dropped, 2^-18 for the lo rounding: p = 2^-17) or rounded once to the plane format (p = 2^-8 / 2^-11; fp16 subnormal weights: 64 * 2^-25
absolute); 3 * 64 (or 64) terms accumulate: with V = max |v| of the window
    |error| <= (2 d + p + 3 * 64 u + 4e-6) V + 10 u S_lepe + fmt |out|        (d per query from its own row of L, S_lepe = sum |w v| + |b|).
sqrelu.  relu(x)^2 is one rounding; with the norm, 1 / rms carries hidden / 2 + 4 roundings and the product one: (hidden / 2 + 6) u + fmt,
relative to each value.
gate_add.  expf within 2 ulp, 1 + e, the division, the fused multiply-add: 8 u (|base| + |kv|) on the f32 map, + fmt |v| on planes.

Shapes are the smallest that reach every path: norm_shift maps of 8 x 8, 16 x 24 and 40 x 72 (the last crosses the 32 x 8 tile edges in both
directions), C 16 / 48 / 128; window grids of 1 x 1 and 2 x 3, C 16 / 48 / 64 / 128 (48: a half-filled last chunk of 32 channels); batch 2;
operands at a plane offset inside a wider buffer whose other planes must come back untouched.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu

U = 2.0**-24
EPS = 2.0**-23


def _fmt_eps(fmt, with_lo):
    return 2.0**-17 if with_lo else (2.0**-11 if fmt == PF_F16 else 2.0**-8)


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _to(pl, device):
    return Planes(pl.hi.to(device), None if pl.lo is None else pl.lo.to(device))


def _back(pl, channels):
    return planes_to_nchw(Planes(pl.hi.cpu(), None if pl.lo is None else pl.lo.cpu()), channels).double()


def _sentinel(n, planes, h, w, device, with_lo, fmt):
    """A plane buffer filled with 3.0 (exact in either format; lo 0.0): planes a kernel must not write come back as 3.0."""
    p = Planes.empty(n, planes, h, w, device, with_lo, fmt)
    p.hi.fill_(3.0)
    if p.lo is not None:
        p.lo.fill_(0.0)
    return p


# ------------------------------------------------------------------------------------------------------------------ norm_shift
def _norm_shift_run(device, c, n, hw, fmt, with_lo, off, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    x = torch.randn((n, c, H, W), generator=g)
    x[0, :, 0, 0] = 0.0  # a pixel of zeros (a corner: its neighbours' taps read it)
    x[0, :, H - 1, W - 1] = torch.randn(c, generator=g) * 1e-4  # eps matters here: mean(x^2) = 1e-8 against 1.2e-7
    x[n - 1, :, H // 2, W // 2] = torch.randn(c, generator=g) * 1e4
    nw = 1.0 + torch.rand(c, generator=g) - 0.5
    w = torch.randn((c, 1, 5, 5), generator=g) / 5  # every tap non-zero, the corners included
    xd = x.double()
    y = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + EPS) * nw.double().reshape(1, c, 1, 1)
    want = F.conv2d(y, w.double(), None, padding=2, groups=c)
    S = F.conv2d(y.abs(), w.double().abs(), None, padding=2, groups=c).max().item()
    planes = off + c // 8 + 1
    out = _sentinel(n, planes, H, W, device, with_lo, fmt)
    xm, nwd, wd = nchw_to_f32map(x).to(device), nw.to(device), w.reshape(c, 25).contiguous().to(device)
    args = lambda xp=xm.data_ptr(), cc=c, ohi=out.hi_ptr(off), e=EPS, bs=out.batch_stride: (  # noqa: E731
        xp, n, H, W, cc, e, nwd.data_ptr(), wd.data_ptr(), ohi, out.lo_ptr(off), out.plane_stride, bs, fmt, _stream(device))  # fmt: skip
    L.check(L.load().rsa_flex_norm_shift(*args()), 'rsa_flex_norm_shift')
    torch.cuda.synchronize()
    full = _back(out, planes * 8)
    assert bool((full[:, : 8 * off] == 3.0).all()) and bool((full[:, 8 * off + c :] == 3.0).all())  # the neighbouring planes are untouched
    return full[:, 8 * off : 8 * off + c], want, S, args, (xm, nwd, wd, out)


@pytest.mark.parametrize('c,n,hw,off', [(16, 2, (8, 8), 1), (48, 1, (16, 24), 0), (128, 1, (8, 8), 2), (16, 2, (40, 72), 1), (48, 1, (9, 35), 0)])
def test_norm_shift(device, c, n, hw, off):
    got, want, S, _, _ = _norm_shift_run(device, c, n, hw, PF_BF16, True, off, c + hw[1])
    err = (got - want).abs().max().item()
    bound = (c / 2 + 30) * U * S + 2.0**-17 * want.abs().max().item()
    print(f'MEASURE flex_norm_shift C={c} n={n} map={hw}: {err:.3e} (bound {bound:.3e}, |out|max {want.abs().max():.2f}, S {S:.2f})')
    assert not got.isnan().any() and err <= bound
    # zero padding of the NORMALISED map: the corner output sees 9 taps only, and the zero pixel contributes nothing
    assert (got[0, :, 0, 0] - want[0, :, 0, 0]).abs().max().item() <= bound


@pytest.mark.parametrize('fmt', [PF_F16, PF_BF16])
def test_norm_shift_hi_planes(device, fmt):
    got, want, S, _, _ = _norm_shift_run(device, 48, 2, (16, 24), fmt, False, 1, 7)
    err = (got - want).abs().max().item()
    bound = (48 / 2 + 30) * U * S + _fmt_eps(fmt, False) * want.abs().max().item()
    print(f'MEASURE flex_norm_shift hi planes fmt={fmt}: {err:.3e} (bound {bound:.3e})')
    assert err <= bound


def test_norm_shift_zero_map_and_bad_arguments(device):
    _, _, _, args, keep = _norm_shift_run(device, 16, 1, (8, 8), PF_BF16, True, 0, 3)
    lib = L.load()
    xm, _, _, out = keep
    zero = torch.zeros_like(xm)
    L.check(lib.rsa_flex_norm_shift(*args(xp=zero.data_ptr())), 'rsa_flex_norm_shift')
    torch.cuda.synchronize()
    assert bool((_back(out, 16 + 8)[:, :16] == 0).all())  # zeros give zeros, not NaN
    assert lib.rsa_flex_norm_shift(*args(cc=12)) == -1
    assert lib.rsa_flex_norm_shift(*args(xp=None)) == -1
    assert lib.rsa_flex_norm_shift(*args(e=-1.0)) == -1
    assert lib.rsa_flex_norm_shift(*args(xp=xm.data_ptr() + 4)) == -3
    assert lib.rsa_flex_norm_shift(*args(ohi=out.hi_ptr() + 8)) == -3
    assert b'flex_norm_shift' in lib.rsa_last_error_string()


# ------------------------------------------------------------------------------------------------------------------ window attention
def _windows(t):
    """[B, C, H, W] -> [B * windows, 64, C]"""
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc, H // 8, 8, W // 8, 8).permute(0, 2, 4, 3, 5, 1).reshape(-1, 64, Cc)


def _attn_run(device, c, n, grid, fmt, products, off, seed):
    g = torch.Generator().manual_seed(seed)
    with_lo = products == 3
    H, W = 8 * grid[0], 8 * grid[1]
    P = c // 8
    planes = off + 3 * P + 1
    x = torch.randn((n, planes * 8, H, W), generator=g)
    q, k, v = (slice(8 * (off + i * P), 8 * (off + (i + 1) * P)) for i in range(3))
    x[:, q] *= 1.5 / c**0.5  # logits of a few units
    x[0, q, 1, 2] *= 40.0  # one query whose logits span more than 100: e^logit overflows f32 without the maximum subtracted
    if n * grid[0] * grid[1] > 1:
        x[n - 1, q, H - 8 :, W - 8 :] = 0.0  # the last window of the last image: all logits equal (q = 0)
    if grid[1] > 1:
        x[:, v, :, 8:16] *= 50.0  # the second window column: a lepe that leaks across a window border shows in its neighbours
    pl = nchw_to_planes(x, with_lo, fmt)
    held = planes_to_nchw(pl, planes * 8).double()
    qw, kw, vw = _windows(held[:, q]), _windows(held[:, k]), _windows(held[:, v])
    lw, lb = torch.randn((c, 1, 3, 3), generator=g) / 3, torch.randn(c, generator=g) * 0.3  # edge taps and bias non-zero
    vi = vw.transpose(1, 2).reshape(-1, c, 8, 8)
    lepe = F.conv2d(vi, lw.double(), lb.double(), padding=1, groups=c).reshape(-1, c, 64).transpose(1, 2)
    s_lepe = F.conv2d(vi.abs(), lw.double().abs(), lb.double().abs(), padding=1, groups=c).reshape(-1, c, 64).transpose(1, 2)
    logits = qw @ kw.transpose(1, 2)
    want = torch.softmax(logits, -1) @ vw + lepe
    assert float((logits[0].max(-1).values - logits[0].min(-1).values).max()) > 100 and not torch.isfinite(torch.exp(logits[0].float())).all()
    Lrow = (qw.abs() @ kw.abs().transpose(1, 2)).max(-1, keepdim=True).values  # [windows, 64, 1]
    V = vw.abs().amax((1, 2), keepdim=True)
    out = _sentinel(n, off + P + 1, H, W, device, with_lo, fmt)
    pd = _to(pl, device)
    lwd, lbd = lw.reshape(c, 9).t().contiguous().to(device), lb.to(device)
    args = lambda hi=pd.hi_ptr(off), lo=pd.lo_ptr(off), cc=c, hh=H, pr=products, ohi=out.hi_ptr(off), bs=pd.batch_stride: (  # noqa: E731
        hi, lo, pd.plane_stride, bs, ohi, out.lo_ptr(off), out.plane_stride, out.batch_stride, n, hh, W, cc, pr, fmt, lwd.data_ptr(), lbd.data_ptr(),
        _stream(device))  # fmt: skip
    L.check(L.load().rsa_flex_window_attn(*args()), 'rsa_flex_window_attn')
    torch.cuda.synchronize()
    full = _back(out, (off + P + 1) * 8)
    assert bool((full[:, : 8 * off] == 3.0).all()) and bool((full[:, 8 * (off + P) :] == 3.0).all())
    got = _windows(full[:, 8 * off : 8 * (off + P)])
    if products == 3:
        d, p, acc = (2.0**-18 + 3 * c * U) * Lrow, 2.0**-17, 3 * 64 * U
    else:
        d, p, acc = c * U * Lrow, (2.0**-11 + 64 * 2.0**-25 if fmt == PF_F16 else 2.0**-8), 64 * U
    bound = (2 * d + p + acc + 4e-6) * V + 10 * U * s_lepe + _fmt_eps(fmt, with_lo) * want.abs()
    return got, want, bound, args, (pd, out, lwd, lbd)


ATTN = [(16, 1, (1, 1), 0), (48, 2, (2, 3), 1), (64, 1, (2, 3), 2), (128, 2, (1, 1), 0), (128, 1, (2, 3), 1)]  # C, batch, windows, plane offset


def _attn_check(tag, got, want, bound):
    err = (got - want).abs()
    worst = (err / bound).max().item()
    print(f'MEASURE flex_window_attn {tag}: max-abs {err.max():.3e} (|out|max {want.abs().max():.2f}), largest error / bound {worst:.3f}')
    assert not got.isnan().any() and worst <= 1.0


@pytest.mark.parametrize('c,n,grid,off', ATTN)
def test_window_attention_three_products(device, c, n, grid, off):
    got, want, bound, _, _ = _attn_run(device, c, n, grid, PF_BF16, 3, off, 11 * c + grid[1])
    _attn_check(f'bf16 hi+lo C={c} n={n} windows={grid}', got, want, bound)


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
@pytest.mark.parametrize('c,n,grid,off', [(16, 2, (1, 1), 1), (48, 1, (2, 3), 0), (64, 2, (2, 3), 1), (128, 1, (1, 1), 2)])
def test_window_attention_one_product(device, c, n, grid, off, fmt):
    got, want, bound, _, _ = _attn_run(device, c, n, grid, fmt, 1, off, 13 * c + grid[1] + fmt)
    _attn_check(f'{"fp16" if fmt == PF_F16 else "bf16"} hi C={c} n={n} windows={grid}', got, want, bound)


def test_window_attention_rejects_bad_arguments(device):
    _, _, _, args, keep = _attn_run(device, 16, 2, (1, 1), PF_BF16, 3, 1, 5)
    lib = L.load()
    pd, out, _, _ = keep
    assert lib.rsa_flex_window_attn(*args(cc=24)) == -1
    assert lib.rsa_flex_window_attn(*args(cc=144)) == -1
    assert lib.rsa_flex_window_attn(*args(hh=12)) == -1
    assert lib.rsa_flex_window_attn(*args(pr=2)) == -1
    assert lib.rsa_flex_window_attn(*args(lo=None)) == -1  # three products need lo planes
    assert lib.rsa_flex_window_attn(*args(bs=1)) == -1
    assert lib.rsa_flex_window_attn(*args(hi=None)) == -1
    assert lib.rsa_flex_window_attn(*args(ohi=pd.hi_ptr(1))) == -1  # in place
    assert lib.rsa_flex_window_attn(*args(hi=pd.hi_ptr(1) + 8)) == -3
    assert b'flex_window_attn' in lib.rsa_last_error_string()
    assert lib.rsa_flex_window_attn_lds_bytes(64, 3) == 18432 and lib.rsa_flex_window_attn_lds_bytes(128, 3) == 36864
    assert lib.rsa_flex_window_attn_lds_bytes(48, 1) == 6912 and lib.rsa_flex_window_attn_lds_bytes(40, 1) == -1


# ------------------------------------------------------------------------------------------------------------------ sqrelu
def _sqrelu_run(device, hidden, norm, inplace, n, hw, fmt, with_lo, off, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    P = hidden // 8
    planes = off + P + 1
    x = torch.randn((n, planes * 8, H, W), generator=g) * 2
    ch = slice(8 * off, 8 * off + hidden)
    x[0, ch, 1, 1] = -x[0, ch, 1, 1].abs() - 0.1  # an all-negative pixel
    pl = nchw_to_planes(x, with_lo, fmt)
    held = planes_to_nchw(pl, planes * 8).double()
    kk = held[:, ch].clamp(min=0) ** 2
    want = kk * torch.rsqrt((kk * kk).mean(1, keepdim=True) + EPS) if norm else kk
    pd = _to(pl, device)
    out = pd if inplace else _sentinel(n, planes, H, W, device, with_lo, fmt)
    args = lambda hi=pd.hi_ptr(off), hid=hidden, ohi=out.hi_ptr(off), ops_=out.plane_stride: (  # noqa: E731
        hi, pd.lo_ptr(off), pd.plane_stride, pd.batch_stride, ohi, out.lo_ptr(off), ops_, out.batch_stride, n, H, W, hid, 1 if norm else 0, EPS, fmt,
        _stream(device))  # fmt: skip
    L.check(L.load().rsa_flex_sqrelu(*args()), 'rsa_flex_sqrelu')
    torch.cuda.synchronize()
    full = _back(out, planes * 8)
    other = held if inplace else torch.full_like(held, 3.0)
    assert torch.equal(full[:, : 8 * off], other[:, : 8 * off]) and torch.equal(full[:, 8 * off + hidden :], other[:, 8 * off + hidden :])
    return full[:, ch], want, args, (pd, out)


@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('hidden,n,hw,off', [(32, 2, (5, 7), 1), (96, 1, (17, 19), 0), (256, 1, (8, 8), 2)])
def test_sqrelu(device, hidden, n, hw, off, norm, inplace):
    got, want, _, _ = _sqrelu_run(device, hidden, norm, inplace, n, hw, PF_BF16, True, off, hidden + 2 * norm + inplace)
    rel = (hidden / 2 + 6) * U + 2.0**-17
    worst = ((got - want).abs() / (rel * want.abs() + 1e-30)).max().item()
    print(f'MEASURE flex_sqrelu hidden={hidden} norm={norm} inplace={inplace}: max-abs {(got - want).abs().max():.3e}, largest error / bound {worst:.3f}')
    assert worst <= 1.0
    assert bool((got[0, :, 1, 1] == 0).all()) and bool((got >= 0).all())  # the all-negative pixel gives zeros


def test_sqrelu_fp16_hi_planes_and_bad_arguments(device):
    got, want, args, keep = _sqrelu_run(device, 32, True, False, 1, (5, 7), PF_F16, False, 1, 4)
    rel = (32 / 2 + 6) * U + 2.0**-11
    assert ((got - want).abs() <= rel * want.abs() + 2.0**-25).all()  # (+ half an fp16 subnormal step)
    lib = L.load()
    pd, _ = keep
    assert lib.rsa_flex_sqrelu(*args(hid=12)) == -1
    assert lib.rsa_flex_sqrelu(*args(hi=None)) == -1
    assert lib.rsa_flex_sqrelu(*args(ohi=pd.hi_ptr(1), ops_=pd.plane_stride + 1)) == -1  # in place with other strides
    assert lib.rsa_flex_sqrelu(*args(hi=pd.hi_ptr(1) + 8)) == -3
    assert b'flex_sqrelu' in lib.rsa_last_error_string()


# ------------------------------------------------------------------------------------------------------------------ gate_add
def _gate_run(device, c, alias, to_planes, n, hw, fmt, with_lo, off, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    P = c // 8
    planes = off + P + 1
    r = torch.randn((n, planes * 8, H, W), generator=g) * 3
    r[0, 8 * off, 0, 0], r[0, 8 * off + 1, 0, 0] = 30.0, -30.0  # both tails of the sigmoid
    kv = torch.randn((n, c, H, W), generator=g)
    base = torch.randn((n, c, H, W), generator=g)
    rp, kp = nchw_to_planes(r, with_lo, fmt), nchw_to_planes(kv, with_lo, fmt)
    rh, kh = planes_to_nchw(rp, planes * 8)[:, 8 * off : 8 * off + c].double(), planes_to_nchw(kp, c).double()
    want = base.double() + torch.sigmoid(rh) * kh
    tol = 8 * U * (base.double().abs() + kh.abs())
    rd, kd = _to(rp, device), _to(kp, device)
    bm = nchw_to_f32map(base).to(device)
    om = bm if alias else torch.full_like(bm, float('nan'))
    op = _sentinel(n, P + 2, H, W, device, with_lo, fmt) if to_planes else None
    args = lambda rhi=rd.hi_ptr(off), cc=c, o=om.data_ptr(), ohi=(op.hi_ptr(1) if op else None), b=bm.data_ptr(): (  # noqa: E731
        rhi, rd.lo_ptr(off), rd.plane_stride, rd.batch_stride, kd.hi_ptr(), kd.lo_ptr(), kd.plane_stride, kd.batch_stride, b, o, ohi,
        op.lo_ptr(1) if op else None, op.plane_stride if op else 0, op.batch_stride if op else 0, n, H, W, cc, fmt, _stream(device))  # fmt: skip
    L.check(L.load().rsa_flex_gate_add(*args()), 'rsa_flex_gate_add')
    torch.cuda.synchronize()
    got = f32map_to_nchw(om.cpu(), c).double()
    gotp = None
    if op:
        full = _back(op, (P + 2) * 8)
        assert bool((full[:, :8] == 3.0).all()) and bool((full[:, 8 + c :] == 3.0).all())
        gotp = full[:, 8 : 8 + c]
    return got, gotp, want, tol, args, (rd, kd, bm, om, op)


@pytest.mark.parametrize('alias', [False, True])
@pytest.mark.parametrize('c,n,hw,off', [(16, 2, (5, 7), 1), (48, 1, (17, 19), 0)])
def test_gate_add(device, c, n, hw, off, alias):
    got, gotp, want, tol, _, _ = _gate_run(device, c, alias, True, n, hw, PF_BF16, True, off, c + alias)
    worst = ((got - want).abs() / tol).max().item()
    worst_p = ((gotp - want).abs() / (tol + 2.0**-17 * want.abs())).max().item()
    print(f'MEASURE flex_gate_add C={c} alias={alias}: max-abs {(got - want).abs().max():.3e}, error / bound: map {worst:.3f}, planes {worst_p:.3f}')
    assert not got.isnan().any() and worst <= 1.0 and worst_p <= 1.0
    # sigmoid(30) = 1 - 9.4e-14 and sigmoid(-30) = 9.4e-14: both tails without overflow
    assert abs(got[0, 0, 0, 0] - want[0, 0, 0, 0]) <= tol[0, 0, 0, 0] and abs(got[0, 1, 0, 0] - want[0, 1, 0, 0]) <= tol[0, 1, 0, 0]


def test_gate_add_one_output_each_and_bad_arguments(device):
    got, _, want, tol, args, keep = _gate_run(device, 16, False, False, 1, (5, 7), PF_F16, False, 1, 2)  # the f32 map alone, fp16 hi planes in
    assert ((got - want).abs() <= tol).all()
    _, gotp, want, tol, args, keep = _gate_run(device, 16, False, True, 1, (5, 7), PF_F16, False, 1, 2)
    rd, _, bm, om, op = keep
    lib = L.load()
    om.fill_(7.0)
    L.check(lib.rsa_flex_gate_add(*args(o=None)), 'rsa_flex_gate_add')  # planes alone
    torch.cuda.synchronize()
    assert bool((om == 7.0).all()) and ((_back(op, 32)[:, 8:24] - want).abs() <= tol + 2.0**-11 * want.abs()).all()
    assert lib.rsa_flex_gate_add(*args(o=None, ohi=None)) == -1  # no output at all
    assert lib.rsa_flex_gate_add(*args(cc=12)) == -1
    assert lib.rsa_flex_gate_add(*args(b=None)) == -1
    assert lib.rsa_flex_gate_add(*args(rhi=rd.hi_ptr(1) + 8)) == -3
    assert lib.rsa_flex_gate_add(*args(o=om.data_ptr() + 4)) == -3
    assert b'flex_gate_add' in lib.rsa_last_error_string()
