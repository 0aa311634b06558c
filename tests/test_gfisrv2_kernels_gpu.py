"""Kernel-level parity of the GFISR family's entry points (csrc/gfisr.hip, csrc/mosr.hip): rsa_gfisr_dft forward and inverse (with and
without post_norm), rsa_gfisr_spectral and rsa_gfisr_gate, and every error code.

Sizes 2x1, 1x2, 5x7, 6x8, 7x70 (wider than a tile), 33x17 and 64x48 (several K steps, ragged M / N tiles); cf 10, 15, 30 and 40 (last planes
with 6, 1, 2 and 0 tail channels); batch 2; both plane formats, with and without lo halves.  Planes sit at an offset inside a larger
sentinel-filled buffer: nothing outside the range may be written.  References are float64 ``torch.fft`` on the CPU, applied to the f32
values the kernel actually read.

Bars:
  f32 outputs of the transform   1e-6 * S per element, S = the sum of absolute input values of that channel times the table scale:
                                 sum|x| / sqrt(HW) forward, sum c_k (|re| + |im|) / sqrt(HW) over the half spectrum inverse.  (An f32-MFMA
                                 product is within 0.75-1.5e-7 * sum|a b| of f64 at K <= 1024, the f32 rounding of a table adds 6e-8, two
                                 passes chain; a CPU f32 matrix DFT sits at 0.4-1.2e-7 * S.)
  planes with lo halves          + 3e-5 * max|ref| (tests/test_moesr_kernels_gpu.py)
  planes without lo halves       + one unit of the format at each reference value's own magnitude
  post_norm                      the transform's bar carried through the norm: |scale| / (rms + eps) * (1 + |y| / (rms + eps)) times the
                                 largest channel's bar, + the plane bar
  rsa_gfisr_spectral, the gate   the plane bars alone (their arithmetic is a handful of f32 operations per value)
The tail channels of a last plane must be exactly zero, and NaN in the unused components of the last group of an f32 map must reach no
output.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gfisr as LG
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map, nchw_to_planes

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
EPS = 1e-6
N = 2
SIZES = [(2, 1), (1, 2), (5, 7), (6, 8), (7, 70), (33, 17), (64, 48)]
CFS = [10, 15, 30, 40]
FORMS = [(PF_BF16, True), (PF_F16, True), (PF_BF16, False), (PF_F16, False)]
# every size with every cf; the plane form cycles so that each size and each cf meets all four
CASES = [(hw, cf, *FORMS[(i + j) % 4]) for i, hw in enumerate(SIZES) for j, cf in enumerate(CFS)]
IDS = [f'{h}x{w}-cf{cf}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for (h, w), cf, f, lo in CASES]
_tabs: dict = {}


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def tables(H, W, device):
    if (H, W) not in _tabs:
        _tabs[(H, W)] = LG.dft_tables(H, W, device)
    return _tabs[(H, W)]


def _unit(ref, fmt):
    """One unit of the plane format at the magnitude of ``ref`` (the spacing of its binade; the subnormal step near zero)."""
    mant, floor = (10, 2.0**-24) if fmt == PF_F16 else (7, 2.0**-133)
    _, e = torch.frexp(ref.abs())
    return torch.clamp(torch.ldexp(torch.ones_like(ref), e - 1 - mant), min=floor)


def _buffer(n, planes, h, w, device, with_lo, fmt, content: Planes | None = None, plane0=1):
    """A sentinel-filled plane buffer with ``planes`` planes of payload from ``plane0`` (two spare planes behind)."""
    P = Planes.empty(n, planes + plane0 + 2, h, w, device, with_lo, fmt)
    P.hi.fill_(SENTINEL)
    if P.lo is not None:
        P.lo.fill_(SENTINEL)
    if content is not None:
        P.hi[:, plane0 : plane0 + planes] = content.hi.to(device)
        if P.lo is not None:
            P.lo[:, plane0 : plane0 + planes] = content.lo.to(device)
    return P


def _read(p: Planes, plane0, planes):
    v = p.hi[:, plane0 : plane0 + planes].double()
    if p.lo is not None:
        v = v + p.lo[:, plane0 : plane0 + planes].double()
    n, _, h, w, _ = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(n, 8 * planes, h, w).cpu()


def _outside_untouched(P: Planes, plane0, planes):
    for t in (P.hi, P.lo) if P.lo is not None else (P.hi,):
        assert (t[:, :plane0] == SENTINEL).all() and (t[:, plane0 + planes :] == SENTINEL).all()


def _plane_bar(ref, fmt, with_lo):
    return torch.full_like(ref, 3e-5 * ref.abs().max().item()) if with_lo else 3e-5 * ref.abs().max().item() + _unit(ref, fmt)


def _dft(device, inverse, H, W, cf, spec, P, plane0, fmt, post=None, override=None):
    tabs = tables(H, W, device)
    nbytes = L.load().rsa_gfisr_dft_scratch_bytes(N, cf, H, W)
    assert nbytes == N * cf * (2 * H * (W // 2 + 1) + H * W) * 4
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    p = LG.GfisrDftParams()
    p.batch, p.H, p.W, p.C, p.inverse, p.fmt, p.eps = N, H, W, cf, int(inverse), fmt, EPS
    p.tab_row, p.tab_col = tabs['row_inv' if inverse else 'row_fwd'].data_ptr(), tabs['col_inv' if inverse else 'col_fwd'].data_ptr()
    p.spec, p.scratch = spec.data_ptr(), scratch.data_ptr()
    if post is not None:
        p.norm_scale, p.norm_offset = post[0].data_ptr(), post[1].data_ptr()
    P.bind(p, 'plane', plane0)
    for k, v in (override or {}).items():
        setattr(p, k, v)
    rc = L.load().rsa_gfisr_dft(C.byref(p), C.c_void_p(ops.current_stream_ptr(device)))
    return rc, scratch


@pytest.mark.parametrize('hw,cf,fmt,with_lo', CASES, ids=IDS)
def test_dft_forward(device, hw, cf, fmt, with_lo):
    H, W = hw
    Wf = W // 2 + 1
    gen = torch.Generator().manual_seed(17 * H + W + cf)
    x = torch.rand(N, cf, H, W, generator=gen) + 2.0  # a large mean: the DC bin is sum / sqrt(HW)
    pl = (cf + 7) // 8
    P = _buffer(N, pl, H, W, device, with_lo, fmt, nchw_to_planes(x, with_lo, fmt))
    before = (P.hi.clone(), None if P.lo is None else P.lo.clone())
    xr = _read(P, 1, pl)[:, :cf]  # what the kernel reads: hi (+ lo), exact in f32
    spec = torch.full((N, (2 * cf + 3) // 4, H, Wf, 4), SENTINEL, device=device)
    rc, _ = _dft(device, False, H, W, cf, spec, P, 1, fmt)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = spec.cpu()
    ref = torch.fft.rfft2(xr, norm='ortho')
    ref = torch.cat([ref.real, ref.imag], 1)  # [real of all cf | imag of all cf]
    S = xr.abs().sum((2, 3), keepdim=True) / (H * W) ** 0.5
    bar = 1e-6 * torch.cat([S, S], 1)
    err = (f32map_to_nchw(got, 2 * cf).double() - ref).abs()
    print(f'MEASURE dft forward {H}x{W} cf {cf}: worst error / S = {(err / torch.cat([S, S], 1)).max().item():.3e} (bar 1e-6)')
    assert (err <= bar).all()
    if (2 * cf) % 4:
        assert (got[:, -1, :, :, (2 * cf) % 4 :] == SENTINEL).all()  # components past 2 cf are not written
    assert torch.equal(P.hi, before[0]) and (P.lo is None or torch.equal(P.lo, before[1]))  # the input is left alone


def _spectrum(H, W, cf, seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 2 * cf, H, W // 2 + 1, generator=gen)  # not Hermitian: the imaginary parts of column 0 and Nyquist are non-zero
    m = nchw_to_f32map(z)
    if (2 * cf) % 4:
        m[:, -1, :, :, (2 * cf) % 4 :] = float('nan')
    zc = torch.complex(z[:, :cf].double(), z[:, cf:].double())
    ck = torch.full((W // 2 + 1,), 2.0, dtype=torch.float64)
    ck[0] = 1.0
    if W % 2 == 0:
        ck[-1] = 1.0
    S = ((z[:, :cf].double().abs() + z[:, cf:].double().abs()) * ck).sum((2, 3), keepdim=True) / (H * W) ** 0.5
    return m, torch.fft.irfft2(zc, s=(H, W), norm='ortho'), S


@pytest.mark.parametrize('hw,cf,fmt,with_lo', CASES, ids=IDS)
def test_dft_inverse(device, hw, cf, fmt, with_lo):
    H, W = hw
    m, ref, S = _spectrum(H, W, cf, 31 * H + W + cf)
    pl = (cf + 7) // 8
    P = _buffer(N, pl, H, W, device, with_lo, fmt)
    spec = m.to(device)
    rc, _ = _dft(device, True, H, W, cf, spec, P, 1, fmt)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = _read(P, 1, pl)
    assert torch.isfinite(got).all()  # the NaN components past 2 cf reached nothing
    err = (got[:, :cf] - ref).abs()
    bar = 1e-6 * S + _plane_bar(ref, fmt, with_lo)
    print(f'MEASURE dft inverse {H}x{W} cf {cf}: worst error / S = {(err / S).max().item():.3e} (f32 bar 1e-6, plane bar {3e-5 * ref.abs().max().item() / S.min().item():.1e} of S)')
    assert (err <= bar).all()
    assert (got[:, cf:] == 0).all()  # the tail channels of the last plane
    _outside_untouched(P, 1, pl)
    assert torch.equal(spec.cpu().nan_to_num(7.0), m.nan_to_num(7.0))  # the input is left alone


@pytest.mark.parametrize('hw,cf,fmt,with_lo', CASES, ids=IDS)
def test_dft_inverse_with_post_norm(device, hw, cf, fmt, with_lo):
    H, W = hw
    m, y, S = _spectrum(H, W, cf, 47 * H + W + cf)
    gen = torch.Generator().manual_seed(cf)
    pl = (cf + 7) // 8
    scale, offset = torch.zeros(8 * pl), torch.zeros(8 * pl)
    scale[:cf], offset[:cf] = 1.0 + 0.25 * torch.randn(cf, generator=gen), 0.1 * torch.randn(cf, generator=gen)
    sc, off = scale[:cf].double()[None, :, None, None], offset[:cf].double()[None, :, None, None]
    rms = y.norm(2, dim=1, keepdim=True) * cf**-0.5
    ref = sc * (y / (rms + EPS)) + off
    P = _buffer(N, pl, H, W, device, with_lo, fmt)
    post = (scale.to(device), offset.to(device))
    rc, _ = _dft(device, True, H, W, cf, m.to(device), P, 1, fmt, post=post)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = _read(P, 1, pl)
    assert torch.isfinite(got).all()
    # d(y_c / rms) <= d / rms * (1 + |y_c| / rms) for an error of at most d in every channel of the pixel (rms moves by at most d too)
    carried = sc.abs() / (rms + EPS) * (1.0 + y.abs() / (rms + EPS)) * (1e-6 * S.max(1, keepdim=True).values)
    err = (got[:, :cf] - ref).abs()
    bar = carried + _plane_bar(ref, fmt, with_lo)
    print(f'MEASURE dft inverse + post_norm {H}x{W} cf {cf}: worst error {err.max().item():.3e}, worst error / bar {(err / bar).max().item():.3f}')
    assert (err <= bar).all()
    assert (got[:, cf:] == 0).all()
    _outside_untouched(P, 1, pl)


SPECTRAL = [((2, 1), 20, True), ((1, 2), 30, False), ((5, 4), 60, True), ((6, 5), 80, False), ((7, 36), 30, True), ((33, 9), 20, False), ((64, 25), 60, True),
            ((9, 70), 80, True)]  # fmt: skip


def _spectral(device, x_map, C_, hw, with_lo, w, b, sc, off, override=None):
    H, W = hw
    pl = (C_ + 7) // 8
    P = _buffer(N, pl, H, W, device, with_lo, PF_BF16)
    keep = [t.to(device).contiguous() for t in (x_map, sc, off, w, b)]
    p = LG.GfisrSpectralParams()
    p.batch, p.H, p.W, p.C, p.eps = N, H, W, C_, EPS
    p.x, p.scale, p.offset, p.weight, p.bias = (t.data_ptr() for t in keep)
    P.bind(p, 'out', 1)
    for k, v in (override or {}).items():
        setattr(p, k, v)
    return L.load().rsa_gfisr_spectral(C.byref(p), C.c_void_p(ops.current_stream_ptr(device))), P, keep


def _spectral_case(hw, C_):
    gen = torch.Generator().manual_seed(1000 * C_ + 7 * hw[0] + hw[1])
    pl8 = 8 * ((C_ + 7) // 8)
    x = torch.randn(N, C_, *hw, generator=gen) * 3.0 + 1.0
    pad = lambda t: torch.cat([t, torch.zeros(pl8 - C_, *t.shape[1:])])  # noqa: E731
    w, b = torch.randn(C_, 9, generator=gen) / 3.0, torch.randn(C_, generator=gen) / 3.0
    sc, off = 1.0 + 0.25 * torch.randn(C_, generator=gen), 0.1 * torch.randn(C_, generator=gen)
    xd = x.double()
    v = sc.double()[None, :, None, None] * (xd / (xd.norm(2, dim=1, keepdim=True) * C_**-0.5 + EPS)) + off.double()[None, :, None, None]
    ref = F.conv2d(v, w.double().reshape(C_, 1, 3, 3), b.double(), padding=1, groups=C_) + v
    m = nchw_to_f32map(x)
    if C_ % 4:
        m[:, -1, :, :, C_ % 4 :] = float('nan')
    return m, pad(w), pad(b), pad(sc), pad(off), ref


@pytest.mark.parametrize('hw,C_,with_lo', SPECTRAL, ids=[f'{h}x{w}-c{c}-{"lo" if lo else "hi"}' for (h, w), c, lo in SPECTRAL])
def test_spectral(device, hw, C_, with_lo):
    m, w, b, sc, off, ref = _spectral_case(hw, C_)
    rc, P, _ = _spectral(device, m, C_, hw, with_lo, w, b, sc, off)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    pl = (C_ + 7) // 8
    got = _read(P, 1, pl)
    assert torch.isfinite(got).all()
    err = (got[:, :C_] - ref).abs()
    bar = _plane_bar(ref, PF_BF16, with_lo)
    print(f'MEASURE spectral {hw[0]}x{hw[1]} C {C_}: worst error {err.max().item():.3e}, worst error / bar {(err / bar).max().item():.3f}')
    assert (err <= bar).all()
    assert (got[:, C_:] == 0).all()
    _outside_untouched(P, 1, pl)


GATE = [((5, 6), PF_BF16, True), ((7, 70), PF_F16, True), ((16, 16), PF_BF16, False), ((9, 33), PF_F16, False)]


def _gate_case(hw, fmt, with_lo, device):
    """MoSRv2-like operands: two passthrough planes (``i`` and the Fourier branch), then 3x3, 1x11 and 11x1 segments of one plane each."""
    H, W = hw
    gen = torch.Generator().manual_seed(5 * H + W)
    planes = 5
    g, x = torch.randn(N, 8 * planes, H, W, generator=gen) * 2.0, torch.randn(N, 8 * planes, H, W, generator=gen)
    G, X = (_buffer(N, planes, H, W, device, with_lo, fmt, nchw_to_planes(t, with_lo, fmt)) for t in (g, x))
    gr, xr = _read(G, 1, planes), _read(X, 1, planes)
    shapes = ((3, 3), (1, 11), (11, 1))
    ws = [torch.randn(8, kh * kw, generator=gen) / (kh * kw) ** 0.5 for kh, kw in shapes]
    bs = [0.1 * torch.randn(8, generator=gen) for _ in shapes]
    parts = [xr[:, :16]]
    for s, (kh, kw) in enumerate(shapes):
        c0 = 16 + 8 * s
        parts.append(F.conv2d(xr[:, c0 : c0 + 8], ws[s].double().reshape(8, 1, kh, kw), bs[s].double(), padding=(kh // 2, kw // 2), groups=8))
    cat = torch.cat(parts, 1)
    keep = [t.to(device).contiguous() for t in ws + bs]
    p = L.GatedDwConvParams()
    p.batch, p.H, p.W, p.fmt, p.i_planes, p.n_segments = N, H, W, fmt, 2, 3
    for s, (kh, kw) in enumerate(shapes):
        p.seg[s].planes, p.seg[s].kh, p.seg[s].kw = 1, kh, kw
        p.seg[s].weight, p.seg[s].bias = keep[s].data_ptr(), keep[3 + s].data_ptr()
    G.bind(p, 'g', 1)
    X.bind(p, 'x', 1)
    return p, gr, cat, planes, (G, X, keep)


@pytest.mark.parametrize('hw,fmt,with_lo', GATE, ids=[f'{h}x{w}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for (h, w), f, lo in GATE])
def test_gate(device, hw, fmt, with_lo):
    p, gr, cat, planes, keep = _gate_case(hw, fmt, with_lo, device)
    lib, stream = L.load(), C.c_void_p(ops.current_stream_ptr(device))
    outs = {}
    for name, call in (('silu', lambda: lib.rsa_gfisr_gate(C.byref(p), L.ACT_SILU, stream)), ('mish', lambda: lib.rsa_gfisr_gate(C.byref(p), L.ACT_MISH, stream)),
                       ('gated_dwconv', lambda: lib.rsa_gated_dwconv(C.byref(p), stream))):  # fmt: skip
        O = _buffer(N, planes, *hw, device, with_lo, fmt)
        O.bind(p, 'out', 1)
        assert call() == 0, lib.rsa_last_error_string()
        torch.cuda.synchronize()
        _outside_untouched(O, 1, planes)
        outs[name] = O
    for name, act in (('silu', F.silu), ('gated_dwconv', F.mish)):
        ref = act(gr) * cat
        err = (_read(outs[name], 1, planes) - ref).abs()
        bar = _plane_bar(ref, fmt, with_lo)
        print(f'MEASURE gate {name} {hw[0]}x{hw[1]}: worst error {err.max().item():.3e}, worst error / bar {(err / bar).max().item():.3f}')
        assert (err <= bar).all()
    # rsa_gated_dwconv is the Mish instance of the one kernel body, bit for bit, and not the SiLU one
    a, b = outs['gated_dwconv'], outs['mish']
    assert torch.equal(a.hi, b.hi) and (a.lo is None or torch.equal(a.lo, b.lo))
    assert not torch.equal(a.hi, outs['silu'].hi)


def test_error_codes(device):
    E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3
    H, W, cf = 5, 7, 10
    m, _, _ = _spectrum(H, W, cf, 1)
    spec = m.to(device)
    post = (torch.ones(16, device=device), torch.zeros(16, device=device))

    def dft(inverse=1, **fields):
        P = _buffer(N, 2, H, W, device, True, PF_BF16, nchw_to_planes(torch.rand(N, cf, H, W), True, PF_BF16))
        return _dft(device, inverse, H, W, cf, spec, P, 1, PF_BF16, post=post if inverse else None, override=fields)[0]

    assert dft(0) == 0 and dft(1) == 0
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(C=0), dict(inverse=2), dict(inverse=-1), dict(reserved0=1), dict(fmt=2), dict(plane_plane_stride=34),
               dict(tab_row=None), dict(tab_col=None), dict(spec=None), dict(scratch=None), dict(plane_hi=None), dict(norm_offset=None), dict(eps=0.0)):  # fmt: skip
        assert dft(**kw) == E_ARG, kw
    assert dft(C=129) == E_UNSUPPORTED and dft(H=40000) == E_UNSUPPORTED
    odd = torch.zeros(64, device=device).data_ptr() + 4
    for key in ('tab_row', 'tab_col', 'spec', 'scratch', 'plane_hi', 'plane_lo', 'norm_scale', 'norm_offset'):
        assert dft(**{key: odd}) == E_ALIGN, key
    assert L.load().rsa_gfisr_dft(None, None) == E_ARG
    assert L.load().rsa_gfisr_dft_scratch_bytes(1, 129, 5, 7) == -1

    ms, w, b, sc, off, _ = _spectral_case((5, 4), 20)
    sp = lambda **fields: _spectral(device, ms, 20, (5, 4), True, w, b, sc, off, override=fields)[0]  # noqa: E731
    assert sp() == 0
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(C=0), dict(eps=0.0), dict(reserved0=1), dict(out_plane_stride=19), dict(x=None), dict(scale=None),
               dict(offset=None), dict(weight=None), dict(bias=None), dict(out_hi=None)):  # fmt: skip
        assert sp(**kw) == E_ARG, kw
    assert sp(C=257) == E_UNSUPPORTED
    for key in ('x', 'scale', 'offset', 'weight', 'bias', 'out_hi', 'out_lo'):
        assert sp(**{key: odd}) == E_ALIGN, key
    assert L.load().rsa_gfisr_spectral(None, None) == E_ARG

    p, _, _, planes, keep = _gate_case((5, 6), PF_BF16, True, device)
    O = _buffer(N, planes, 5, 6, device, True, PF_BF16)
    O.bind(p, 'out', 1)
    lib, stream = L.load(), C.c_void_p(ops.current_stream_ptr(device))
    assert lib.rsa_gfisr_gate(C.byref(p), L.ACT_SILU, stream) == 0
    for act in (L.ACT_NONE, L.ACT_LRELU, L.ACT_GELU, 7, -1):
        assert lib.rsa_gfisr_gate(C.byref(p), act, stream) == E_UNSUPPORTED, act
    assert lib.rsa_gfisr_gate(None, L.ACT_SILU, stream) == E_ARG
    p.seg[0].kh = 4
    assert lib.rsa_gfisr_gate(C.byref(p), L.ACT_SILU, stream) == E_UNSUPPORTED
    p.seg[0].kh, p.n_segments = 3, 5
    assert lib.rsa_gfisr_gate(C.byref(p), L.ACT_SILU, stream) == E_ARG
    p.n_segments, p.out_hi = 3, odd
    assert lib.rsa_gfisr_gate(C.byref(p), L.ACT_SILU, stream) == E_ALIGN
    torch.cuda.synchronize()
