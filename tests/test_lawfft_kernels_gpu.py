"""Kernel-level parity of the LAWFFT entry points (csrc/lawfft.hip), each alone, through the C-ABI, against float64 on the values the
kernel read: rsa_lawfft_wincorr, rsa_lawfft_norm_mul, rsa_lawfft_spec_mul, the whole-image chain (rsa_gfisr_dft forward twice, the
multiply, rsa_gfisr_dft inverse), rsa_lawfft_kernel_gen and rsa_lawfft_dyn_dwconv.

Planes sit at an offset inside a larger sentinel-filled buffer (q, k, v and the output at different offsets, so their batch strides
differ): nothing outside the range may be written.  Where C is no multiple of 8 the tail channels of every input's last plane are NaN:
they must reach no output, and the output's tail channels must be exactly zero.  Every case runs twice and must give the same bits.

Bars.  None of these kernels shares its arithmetic with an older one except the transforms of the chain, so, as measured per case on the
CPU: 4 x the largest deviation of torch's own f32 computation of the same expression from float64 on the same inputs (another summation
order), plus the rounding of the output format -- tests/test_gfisrv2_kernels_gpu.py's plane bar (3e-5 max|ref| with lo halves, one unit
of the format more without), 2^-23 max|ref| for an f32 output.  The chain takes rsa_gfisr_dft's bar, 1e-6 S per transform with S the
absolute sum the transform runs over, carried through the product: with E_q = 1e-6 sum|q| / sqrt(HW) (E_k likewise) on every bin of the
two ortho spectra, a bin of their product is off by at most E_q (|K_re| + |K_im|) + E_k (|Q_re| + |Q_im|) in either part; the inverse sums
the bins with irfft2's weights c_k and adds its own 1e-6 sum c_k (|P_re| + |P_im|); sqrt(HW) / sqrt(HW) cancels.  Then the plane bar.
rsa_lawfft_wincorr on integer-valued q and k computes corr exactly, as float64 does: fed to rsa_lawfft_norm_mul as planes, the two
epilogues must agree bit for bit.  Every case prints a MEASURE line; profiles/lawfft_kernels_measure.txt keeps them.
"""

import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_lawfft as LW
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, f32map_to_nchw, nchw_to_f32map, nchw_to_planes
from test_gfisrv2_kernels_gpu import SENTINEL, _buffer, _dft, _outside_untouched, _plane_bar, _read

pytestmark = pytest.mark.gpu

N = 2
EPS = 1e-6
FORMS = [(PF_BF16, True), (PF_F16, True), (PF_BF16, False), (PF_F16, False)]
MAPS = [(8, 8), (16, 24), (40, 8)]  # one patch; several patches in both directions; a tall strip
CS = [1, 8, 45, 128]
WIN_CASES = [(hw, c, *FORMS[(i + j) % 4]) for i, hw in enumerate(MAPS) for j, c in enumerate(CS)]
WIN_IDS = [f'{h}x{w}-c{c}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for (h, w), c, f, lo in WIN_CASES]


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _fmt(fmt, lo):
    return f'{"f16" if fmt == PF_F16 else "bf16"}-{"lo" if lo else "hi"}'


def _planes_of(x, device, fmt, with_lo, plane0, n=N):
    """``x`` [n, C, H, W] as planes from ``plane0`` of a sentinel buffer, the tail channels of the last plane NaN; and what a kernel reads."""
    c = x.shape[1]
    pl = (c + 7) // 8
    P = _buffer(n, pl, *x.shape[2:], device, with_lo, fmt, nchw_to_planes(x, with_lo, fmt), plane0=plane0)
    if c % 8:
        for t in (P.hi, P.lo) if with_lo else (P.hi,):
            t[:, plane0 + pl - 1, :, :, c % 8 :] = float('nan')
    return P, _read(P, plane0, pl)[:, :c]


def _layer_norm(x, w, b):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[None, :, None, None] * ((x - u) / torch.sqrt(s + EPS)) + b[None, :, None, None]


def _patches(x):
    b, c, h, w = x.shape
    return x.view(b, c, h // 8, 8, w // 8, 8).permute(0, 1, 2, 4, 3, 5)


def _unpatch(x):
    b, c, nh, nw, _, _ = x.shape
    return x.permute(0, 1, 2, 4, 3, 5).reshape(b, c, nh * 8, nw * 8)


def _wincorr_ref(q, k, v, w, b):
    """The expression as the model states it, in the dtype of the inputs."""
    corr = _unpatch(torch.fft.irfft2(torch.fft.rfft2(_patches(q)) * torch.fft.rfft2(_patches(k)), s=(8, 8)))
    return v * _layer_norm(corr, w, b)


def _check_planes(what, O, plane0, c, ref, dev, fmt, with_lo):
    pl = (c + 7) // 8
    got = _read(O, plane0, pl)
    assert torch.isfinite(got).all(), f'{what}: a NaN of a tail channel reached the output'
    err = (got[:, :c] - ref).abs()
    bar = 4 * dev + _plane_bar(ref, fmt, with_lo)
    print(f'MEASURE {what}: max-abs {err.max().item():.3e} (|ref|max {ref.abs().max().item():.3f}; torch f32 - f64 {dev:.2e}; worst error / bar {(err / bar).max().item():.3f})')
    assert (err <= bar).all(), what
    assert (got[:, c:] == 0).all(), f'{what}: tail channels must be zero'
    _outside_untouched(O, plane0, pl)


def _wincorr(device, H, W, c, fmt, Q, K, V, O, w, b, offs=(1, 2, 3, 1)):
    p = LW.LawfftWincorrParams()
    p.batch, p.H, p.W, p.C, p.fmt, p.eps = Q.n, H, W, c, fmt, EPS
    p.weight, p.bias = w.data_ptr(), b.data_ptr()
    for name, P, off in zip(('q', 'k', 'v', 'out'), (Q, K, V, O), offs):
        P.bind(p, name, off)
    assert L.load().rsa_lawfft_wincorr(C.byref(p), _stream(device)) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()


def _norm_mul(device, H, W, c, corr_fmt, fmt, CR, V, O, w, b, offs=(2, 3, 1)):
    p = LW.LawfftNormMulParams()
    p.batch, p.H, p.W, p.C, p.corr_fmt, p.fmt, p.eps = CR.n, H, W, c, corr_fmt, fmt, EPS
    p.weight, p.bias = w.data_ptr(), b.data_ptr()
    for name, P, off in zip(('corr', 'v', 'out'), (CR, V, O), offs):
        P.bind(p, name, off)
    assert L.load().rsa_lawfft_norm_mul(C.byref(p), _stream(device)) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()


def _affine(c, gen, device):
    pl8 = 8 * ((c + 7) // 8)
    w, b = torch.full((pl8,), float('nan')), torch.full((pl8,), float('nan'))  # past C: never read as values
    w[:c], b[:c] = 1.0 + 0.25 * torch.randn(c, generator=gen), 0.1 * torch.randn(c, generator=gen)
    return w.to(device), b.to(device), w[:c].double(), b[:c].double()


def _twice(run, O):
    run()
    first = (O.hi.clone(), None if O.lo is None else O.lo.clone())
    O.hi.fill_(SENTINEL)
    if O.lo is not None:
        O.lo.fill_(SENTINEL)
    run()
    # (bit patterns: a NaN would compare unequal to itself, and none may be there)
    assert torch.equal(O.hi.view(torch.int16), first[0].view(torch.int16)) and (O.lo is None or torch.equal(O.lo.view(torch.int16), first[1].view(torch.int16)))


@pytest.mark.parametrize('hw,c,fmt,with_lo', WIN_CASES, ids=WIN_IDS)
def test_wincorr(device, hw, c, fmt, with_lo):
    H, W = hw
    gen = torch.Generator().manual_seed(100 * H + W + c)
    q, k, v = (torch.randn(N, c, H, W, generator=gen) for _ in range(3))
    (Q, qr), (K, kr), (V, vr) = (_planes_of(t, device, fmt, with_lo, off) for t, off in ((q, 1), (k, 2), (v, 3)))
    assert len({Q.batch_stride, K.batch_stride, V.batch_stride}) == 3
    w, b, w64, b64 = _affine(c, gen, device)
    O = _buffer(N, (c + 7) // 8, H, W, device, with_lo, fmt)
    _twice(lambda: _wincorr(device, H, W, c, fmt, Q, K, V, O, w, b), O)
    ref = _wincorr_ref(qr, kr, vr, w64, b64)
    dev = (_wincorr_ref(qr.float(), kr.float(), vr.float(), w64.float(), b64.float()).double() - ref).abs().max().item()
    _check_planes(f'wincorr {H}x{W} c {c} {_fmt(fmt, with_lo)}', O, 1, c, ref, dev, fmt, with_lo)


@pytest.mark.parametrize('hw,c,fmt,with_lo', WIN_CASES, ids=WIN_IDS)
def test_norm_mul(device, hw, c, fmt, with_lo):
    H, W = hw
    gen = torch.Generator().manual_seed(200 * H + W + c)
    corr, v = 3.0 * torch.randn(N, c, H, W, generator=gen) + 1.0, torch.randn(N, c, H, W, generator=gen)
    # the correlation arrives as bf16 hi + lo planes in the model whatever the policy: every other case reads that form beside its own
    corr_fmt, corr_lo = (PF_BF16, True) if (H + c) % 2 else (fmt, with_lo)
    (CR, cr), (V, vr) = _planes_of(corr, device, corr_fmt, corr_lo, 2), _planes_of(v, device, fmt, with_lo, 3)
    w, b, w64, b64 = _affine(c, gen, device)
    O = _buffer(N, (c + 7) // 8, H, W, device, with_lo, fmt)
    _twice(lambda: _norm_mul(device, H, W, c, corr_fmt, fmt, CR, V, O, w, b), O)
    ref = vr * _layer_norm(cr, w64, b64)
    dev = ((vr.float() * _layer_norm(cr.float(), w64.float(), b64.float())).double() - ref).abs().max().item()
    _check_planes(f'norm_mul {H}x{W} c {c} corr {_fmt(corr_fmt, corr_lo)} -> {_fmt(fmt, with_lo)}', O, 1, c, ref, dev, fmt, with_lo)


@pytest.mark.parametrize('fmt,with_lo', FORMS, ids=[_fmt(*f) for f in FORMS])
@pytest.mark.parametrize('c', [8, 45])
def test_wincorr_epilogue_is_norm_mul_bit_for_bit(device, c, fmt, with_lo):
    """q and k in {-1, 0, 1}: every correlation is an integer of at most 64 in magnitude, exact in f32 and in every plane form, so
    rsa_lawfft_norm_mul reads from planes exactly what rsa_lawfft_wincorr holds in LDS."""
    H, W = 16, 24
    gen = torch.Generator().manual_seed(7 * c + fmt)
    q, k = (torch.randint(-1, 2, (N, c, H, W), generator=gen).float() for _ in range(2))
    v = torch.randn(N, c, H, W, generator=gen)
    (Q, qr), (K, kr), (V, _) = (_planes_of(t, device, fmt, with_lo, off) for t, off in ((q, 1), (k, 2), (v, 3)))
    corr = _unpatch(torch.fft.irfft2(torch.fft.rfft2(_patches(qr)) * torch.fft.rfft2(_patches(kr)), s=(8, 8))).round()
    assert corr.abs().max() <= 64
    CR, cr = _planes_of(corr.float(), device, fmt, with_lo, 2)
    assert torch.equal(cr, corr)  # float64-exact in the planes
    w, b, _, _ = _affine(c, gen, device)
    O1, O2 = (_buffer(N, (c + 7) // 8, H, W, device, with_lo, fmt) for _ in range(2))
    _wincorr(device, H, W, c, fmt, Q, K, V, O1, w, b)
    _norm_mul(device, H, W, c, fmt, fmt, CR, V, O2, w, b)
    assert torch.equal(O1.hi.view(torch.int16), O2.hi.view(torch.int16))
    assert O1.lo is None or torch.equal(O1.lo.view(torch.int16), O2.lo.view(torch.int16))


# ---------------------------------------------------------------- rsa_lawfft_spec_mul
def _spec(c, H, Wf, gen):
    z = torch.randn(N, 2 * c, H, Wf, generator=gen)
    m = nchw_to_f32map(z)
    if (2 * c) % 4:
        m[:, -1, :, :, (2 * c) % 4 :] = float('nan')
    return z, m


def _spec_mul(device, c, H, Wf, scale, a, b, out):
    p = LW.LawfftSpecMulParams()
    p.batch, p.H, p.W, p.C, p.scale = N, H, Wf, c, scale
    p.a, p.b, p.out = a.data_ptr(), b.data_ptr(), out.data_ptr()
    assert L.load().rsa_lawfft_spec_mul(C.byref(p), _stream(device)) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('unit_scale', [True, False], ids=['scale1', 'scale-sqrtHW'])
@pytest.mark.parametrize('hw', [(8, 5), (16, 13)], ids=['8x5', '16x13'])
@pytest.mark.parametrize('c', [1, 3, 45, 128])
def test_spec_mul(device, c, hw, unit_scale, in_place):
    H, Wf = hw
    scale = 1.0 if unit_scale else math.sqrt(H * 2 * (Wf - 1))
    gen = torch.Generator().manual_seed(1000 * c + 10 * H + Wf)
    (za, ma), (zb, mb) = _spec(c, H, Wf, gen), _spec(c, H, Wf, gen)
    b = mb.to(device)

    def run():
        a = ma.to(device)
        out = a if in_place else torch.full_like(a, SENTINEL)
        _spec_mul(device, c, H, Wf, scale, a, b, out)
        return a.cpu(), out.cpu()

    a_after, got = run()
    s32 = torch.tensor(scale, dtype=torch.float32)
    ref = s32.double() * (torch.complex(za[:, :c].double(), za[:, c:].double()) * torch.complex(zb[:, :c].double(), zb[:, c:].double()))
    ref = torch.cat([ref.real, ref.imag], 1)
    t32 = s32 * (torch.complex(za[:, :c], za[:, c:]) * torch.complex(zb[:, :c], zb[:, c:]))
    dev = (torch.cat([t32.real, t32.imag], 1).double() - ref).abs().max().item()
    err = (f32map_to_nchw(got, 2 * c).double() - ref).abs()
    bar = 4 * dev + 2.0**-23 * ref.abs().max().item()
    print(f'MEASURE spec_mul c {c} {H}x{Wf} scale {scale:.3f} {"in place" if in_place else "out of place"}: max-abs {err.max().item():.3e} (|ref|max {ref.abs().max().item():.2f}; torch f32 - f64 {dev:.2e}; bar {bar:.2e})')
    assert (err <= bar).all()
    if (2 * c) % 4:  # components past 2 C are not written: still the sentinel, or the NaN the input had
        tail = got[:, -1, :, :, (2 * c) % 4 :]
        assert tail.isnan().all() if in_place else (tail == SENTINEL).all()
    assert torch.equal(b.cpu().nan_to_num(7.0), mb.nan_to_num(7.0)) and (in_place or torch.equal(a_after.nan_to_num(7.0), ma.nan_to_num(7.0)))
    assert torch.equal(run()[1].nan_to_num(7.0), got.nan_to_num(7.0))  # the second run: the same bits


# ---------------------------------------------------------------- the whole-image chain
CHAIN = [((8, 8), 45, PF_BF16, True), ((16, 24), 45, PF_F16, True), ((24, 40), 45, PF_BF16, True), ((16, 24), 8, PF_BF16, False), ((24, 40), 128, PF_F16, False)]


@pytest.mark.parametrize('hw,c,fmt,with_lo', CHAIN, ids=[f'{h}x{w}-c{c}-{_fmt(f, lo)}' for (h, w), c, f, lo in CHAIN])
def test_whole_image_chain_against_torch_fft(device, hw, c, fmt, with_lo):
    H, W = hw
    Wf = W // 2 + 1
    gen = torch.Generator().manual_seed(300 * H + W + c)
    q, k = torch.randn(N, c, H, W, generator=gen), torch.randn(N, c, H, W, generator=gen)
    (Q, qr), (K, kr) = _planes_of(q, device, fmt, with_lo, 1), _planes_of(k, device, fmt, with_lo, 1)
    A, B = (torch.full((N, (2 * c + 3) // 4, H, Wf, 4), SENTINEL, device=device) for _ in range(2))
    O = _buffer(N, (c + 7) // 8, H, W, device, True, PF_BF16)  # the correlation is written as bf16 hi + lo planes in every policy
    assert _dft(device, False, H, W, c, A, Q, 1, fmt)[0] == 0 and _dft(device, False, H, W, c, B, K, 1, fmt)[0] == 0
    _spec_mul(device, c, H, Wf, math.sqrt(H * W), A, B, A)
    rc, _ = _dft(device, True, H, W, c, A, O, 1, PF_BF16)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    ref = torch.fft.irfft2(torch.fft.rfft2(qr) * torch.fft.rfft2(kr))  # torch's default 'backward' normalisation
    assert ref.shape[-2:] == (H, W)
    Qo, Ko = torch.fft.rfft2(qr, norm='ortho'), torch.fft.rfft2(kr, norm='ortho')
    ck = torch.full((Wf,), 2.0, dtype=torch.float64)
    ck[0] = ck[-1] = 1.0  # W is even
    l1 = lambda z: z.real.abs() + z.imag.abs()  # noqa: E731
    Eq, Ek = (1e-6 * t.abs().sum((2, 3), keepdim=True) / (H * W) ** 0.5 for t in (qr, kr))
    bound = (2 * ck * (Eq * l1(Ko) + Ek * l1(Qo))).sum((2, 3), keepdim=True) + 1e-6 * (ck * l1(Qo * Ko)).sum((2, 3), keepdim=True)
    got = _read(O, 1, (c + 7) // 8)
    assert torch.isfinite(got).all()
    err = (got[:, :c] - ref).abs()
    bar = bound + _plane_bar(ref, PF_BF16, True)
    print(f'MEASURE whole-image chain {H}x{W} c {c} {_fmt(fmt, with_lo)}: max-abs {err.max().item():.3e} (|ref|max {ref.abs().max().item():.2f}; worst error / transform bound {(err / bound).max().item():.3f}; worst error / bar {(err / bar).max().item():.3f})')
    assert (err <= bar).all()
    assert (got[:, c:] == 0).all()
    _outside_untouched(O, 1, (c + 7) // 8)


# ---------------------------------------------------------------- rsa_lawfft_kernel_gen
GEN_CASES = [(c, k, hw, *FORMS[(i + j + m) % 4]) for i, c in enumerate([1, 15, 16, 60, 128]) for j, k in enumerate([3, 5]) for m, hw in enumerate([(8, 8), (24, 40)])]
B3 = 3


def _gen(device, c, k, H, W, fmt, P, plane0, w1, b1, w2, b2, out):
    lib = L.load()
    packed = [t.to(device) for t in LW.pack_kernel_gen(w1, b1, w2, b2)]
    nbytes = lib.rsa_lawfft_kernel_gen_workspace_bytes(B3, c, H, W)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes // 4,), float('nan'), device=device)
    p = LW.LawfftKernelGenParams()
    p.batch, p.H, p.W, p.C, p.ksize, p.fmt = B3, H, W, c, k, fmt
    p.w1_t, p.b1, p.w2_t, p.b2 = (t.data_ptr() for t in packed)
    p.workspace, p.out = ws.data_ptr(), out.data_ptr()
    P.bind(p, 'in', plane0)
    assert lib.rsa_lawfft_kernel_gen(C.byref(p), _stream(device)) == 0, lib.rsa_last_error_string()
    torch.cuda.synchronize()


def _gen_ref(x, w1, b1, w2, b2):
    m = x.mean((2, 3))
    return F.linear(F.relu(F.linear(m, w1.reshape(w1.shape[0], -1), b1)), w2.reshape(w2.shape[0], -1), b2)


def _kernel_gen_case(device, c, k, hw, fmt, with_lo, dead):
    H, W = hw
    gen = torch.Generator().manual_seed(10 * c + k + H)
    x = torch.randn(B3, c, H, W, generator=gen) + torch.randn(B3, c, 1, 1, generator=gen)  # three different images, three different means
    P, xr = _planes_of(x, device, fmt, with_lo, 1, n=B3)
    w1, b1 = torch.randn(c, c, 1, 1, generator=gen), torch.randn(c, generator=gen) - (100.0 if dead else 0.0)
    w2, b2 = torch.randn(c * k * k, c, 1, 1, generator=gen) / c**0.5, torch.randn(c * k * k, generator=gen)
    pl8 = 8 * ((c + 7) // 8)
    out = torch.full((B3, pl8, k * k), SENTINEL, device=device)
    _gen(device, c, k, H, W, fmt, P, 1, w1, b1, w2, b2, out)
    got = out.cpu()
    ref = _gen_ref(xr, w1.double(), b1.double(), w2.double(), b2.double()).reshape(B3, c, k * k)
    dev = (_gen_ref(xr.float(), w1, b1, w2, b2).reshape(B3, c, k * k).double() - ref).abs().max().item()
    err = (got[:, :c].double() - ref).abs().max().item()
    bar = 4 * dev + 2.0**-23 * ref.abs().max().item()
    hidden = F.linear(xr.mean((2, 3)), w1.double().reshape(c, c), b1.double())
    print(f'MEASURE kernel_gen c {c} k {k} {H}x{W} {_fmt(fmt, with_lo)}{" dead" if dead else ""}: max-abs {err:.3e} (|ref|max {ref.abs().max().item():.2f}; torch f32 - f64 {dev:.2e}; bar {bar:.2e}; {int((hidden > 0).sum())} of {hidden.numel()} hidden units active)')
    assert err <= bar
    assert (got[:, c:] == 0).all() and torch.isfinite(got).all()
    if dead:
        assert (hidden < 0).all() and torch.equal(got[:, :c], b2.reshape(1, c, k * k).expand(B3, -1, -1))  # b2 alone, exactly
    elif c > 1:
        assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])  # one kernel set per sample
    out2 = torch.full_like(out, SENTINEL)
    _gen(device, c, k, H, W, fmt, P, 1, w1, b1, w2, b2, out2)
    assert torch.equal(out2.cpu(), got)


# ---------------------------------------------------------------- rsa_lawfft_dyn_dwconv
DYN_CASES = [(k, hw, c, *FORMS[(i + j + m) % 4]) for i, k in enumerate([3, 5]) for j, hw in enumerate([(8, 8), (16, 24)]) for m, c in enumerate([15, 64])]


def _dyn(device, c, k, H, W, fmt, P, O, weight, res1=None, res2=None, out_f32=None, n=N):
    p = LW.LawfftDynDwConvParams()
    p.batch, p.H, p.W, p.C, p.ksize, p.fmt = n, H, W, c, k, fmt
    p.weight = weight.data_ptr()
    p.res1, p.res2, p.out_f32 = (None if t is None else t.data_ptr() for t in (res1, res2, out_f32))
    P.bind(p, 'in', 1)
    if O is not None:
        O.bind(p, 'out', 2)
    assert L.load().rsa_lawfft_dyn_dwconv(C.byref(p), _stream(device)) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()


def _dyn_ref(x, kern, k):
    n, c, H, W = x.shape
    return F.conv2d(x.reshape(1, n * c, H, W), kern.reshape(n * c, 1, k, k), padding=k // 2, groups=n * c).reshape(n, c, H, W)


def _dyn_weights(c, k, gen, device):
    pl8 = 8 * ((c + 7) // 8)
    kern = torch.randn(N, c, k * k, generator=gen) / k
    wt = torch.full((N, pl8, k * k), float('nan'))  # past C: the generator writes zeros there, and nothing may depend on it
    wt[:, :c] = kern
    return kern, wt.to(device)


@pytest.mark.parametrize('k,hw,c,fmt,with_lo', DYN_CASES, ids=[f'k{k}-{h}x{w}-c{c}-{_fmt(f, lo)}' for k, (h, w), c, f, lo in DYN_CASES])
def test_dyn_dwconv(device, k, hw, c, fmt, with_lo):
    H, W = hw
    gen = torch.Generator().manual_seed(50 * k + H + c)
    x = torch.randn(N, c, H, W, generator=gen)
    P, xr = _planes_of(x, device, fmt, with_lo, 1)
    kern, wt = _dyn_weights(c, k, gen, device)
    O = _buffer(N, (c + 7) // 8, H, W, device, with_lo, fmt, plane0=2)
    _twice(lambda: _dyn(device, c, k, H, W, fmt, P, O, wt), O)
    ref = _dyn_ref(xr, kern.double(), k)
    dev = (_dyn_ref(xr.float(), kern, k).double() - ref).abs().max().item()
    assert not torch.allclose(_dyn_ref(xr[:1], kern[1:].double(), k), ref[:1])  # the two samples' kernels differ: sharing them would show
    _check_planes(f'dyn_dwconv k {k} {H}x{W} c {c} {_fmt(fmt, with_lo)}', O, 2, c, ref, dev, fmt, with_lo)


@pytest.mark.parametrize('c,planes_out', [(15, True), (60, False), (30, True)], ids=['c15-planes+f32', 'c60-f32-only', 'c30-planes+f32'])
def test_dyn_dwconv_residuals_and_f32_output(device, c, planes_out):
    k, H, W, fmt, with_lo = 3, 16, 24, PF_BF16, True
    gen = torch.Generator().manual_seed(c)
    x, r1, r2 = (torch.randn(N, c, H, W, generator=gen) for _ in range(3))
    P, xr = _planes_of(x, device, fmt, with_lo, 1)
    kern, wt = _dyn_weights(c, k, gen, device)
    m1, m2 = nchw_to_f32map(r1), nchw_to_f32map(r2)
    if c % 4:
        m1[:, -1, :, :, c % 4 :] = float('nan')
    O = _buffer(N, (c + 7) // 8, H, W, device, with_lo, fmt, plane0=2) if planes_out else None
    out32 = torch.full_like(m1, SENTINEL).to(device)
    _dyn(device, c, k, H, W, fmt, P, O, wt, res1=m1.to(device), res2=m2.to(device), out_f32=out32)
    ref = _dyn_ref(xr, kern.double(), k) + r1.double() + r2.double()
    dev = ((_dyn_ref(xr.float(), kern, k) + r1 + r2).double() - ref).abs().max().item()
    got32 = out32.cpu()
    err = (f32map_to_nchw(got32, c).double() - ref).abs().max().item()
    bar = 4 * dev + 2.0**-23 * ref.abs().max().item()
    print(f'MEASURE dyn_dwconv + two residuals -> f32 map, c {c}: max-abs {err:.3e} (torch f32 - f64 {dev:.2e}; bar {bar:.2e})')
    assert err <= bar and torch.isfinite(got32).all()
    if c % 4:
        assert (got32[:, -1, :, :, c % 4 :] == 0).all()
    if planes_out:
        _check_planes(f'dyn_dwconv + two residuals -> planes, c {c}', O, 2, c, ref, dev, fmt, with_lo)


@pytest.mark.parametrize('c,k,hw,fmt,with_lo', GEN_CASES, ids=[f'c{c}-k{k}-{h}x{w}-{_fmt(f, lo)}' for c, k, (h, w), f, lo in GEN_CASES])
def test_kernel_gen(device, c, k, hw, fmt, with_lo):
    _kernel_gen_case(device, c, k, hw, fmt, with_lo, dead=False)


def test_kernel_gen_with_every_hidden_unit_negative(device):
    """The ReLU is all-zero: b2 alone is the output, exactly."""
    _kernel_gen_case(device, 15, 5, (24, 40), PF_BF16, True, dead=True)
