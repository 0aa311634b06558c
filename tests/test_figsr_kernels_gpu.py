"""Kernel-level parity of the FIGSR entry points (csrc/figsr.hip): rsa_figsr_mix against float64 ``F.conv2d`` + SiLU on the values the
kernel read, and against the composition it replaces (two rsa_plk_conv launches with each band embedded in a zero K x K kernel, then
rsa_gfisr_gate); rsa_figsr_input and rsa_figsr_output against torch; every error code.

rsa_figsr_mix: sizes 3x5 and 5x3 (the band is mostly outside the image), 6x8, 7x70 (wider than a tile), 17x33 and 33x17 (one past the
16 x 32 tile), 64x48; K 3, 11, 17, 31; gc 8 and 16; 0 and 5 pass-through planes; batch 2; bf16 planes in three products (hi + lo), fp16
planes in one product with and without lo halves -- the (format, products) pairs the kernel is compiled for, as rsa_plk_conv.  Every size
meets every K; gc, the pass-through count and the plane form cycle so that each size and each K meets all of them.  Planes sit at an
offset inside a larger sentinel-filled buffer: nothing outside the range may be written.

Bars, the project's own for this arithmetic:
  the convolution term     1e-5 * max|conv| in three products, 2e-3 * max|conv| in one (tests/test_plksr_kernels_gpu.py), times |silu(g)|
  planes with lo halves    + 3e-5 * max|ref|                                         (tests/test_gfisrv2_kernels_gpu.py)
  planes without           + 3e-5 * max|ref| + one unit of the format at each reference value's own magnitude
  against the composition  twice the plane bar (two roundings to planes there, one here; the same products, another summation order)
  input / output           the plane bars alone / one rounding of the output dtype
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_figsr as LF
from resselt_amd.engine import lib_gfisr  # noqa: F401  (registers rsa_gfisr_gate)
from resselt_amd.engine import ops, plk
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, nchw_to_planes
from test_gfisrv2_kernels_gpu import SENTINEL, _buffer, _outside_untouched, _plane_bar, _read

pytestmark = pytest.mark.gpu

N = 2
E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3
SIZES = [(3, 5), (5, 3), (6, 8), (7, 70), (17, 33), (33, 17), (64, 48)]
KS = [3, 11, 17, 31]
FORMS = [(PF_BF16, True), (PF_F16, True), (PF_F16, False)]  # (format, lo halves): three products on bf16 hi + lo, one product on fp16
CASES = [(hw, k, (8, 16)[(i + j) % 2], (0, 5)[((i + j) // 2 + j) % 2], *FORMS[(i + 2 * j) % 3]) for i, hw in enumerate(SIZES) for j, k in enumerate(KS)]
IDS = [f'{h}x{w}-k{k}-gc{gc}-pass{ps}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for (h, w), k, gc, ps, f, lo in CASES]


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def test_the_cases_cover_every_axis():
    for hw in SIZES:
        assert {c[1] for c in CASES if c[0] == hw} == set(KS)
        assert {c[2] for c in CASES if c[0] == hw} == {8, 16} and {c[3] for c in CASES if c[0] == hw} == {0, 5}
        assert len({c[4:] for c in CASES if c[0] == hw}) == 3
    for k in KS:
        assert {c[2] for c in CASES if c[1] == k} == {8, 16} and {c[3] for c in CASES if c[1] == k} == {0, 5} and len({c[4:] for c in CASES if c[1] == k}) == 3


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _mix_case(device, hw, k, gc, ps, fmt, with_lo):
    H, W = hw
    P = gc // 8
    planes = ps + 3 * P
    products = 3 if fmt == PF_BF16 else 1
    gen = torch.Generator().manual_seed(1000 * k + 10 * H + W + gc + ps)
    g = torch.randn(N, 8 * planes, H, W, generator=gen) * 2.0
    x = torch.randn(N, 8 * planes, H, W, generator=gen)
    hw_t = torch.randn(N, gc, H, W, generator=gen)
    G, X = (_buffer(N, planes, H, W, device, with_lo, fmt, nchw_to_planes(t, with_lo, fmt)) for t in (g, x))
    HWp = _buffer(N, P, H, W, device, with_lo, fmt, nchw_to_planes(hw_t, with_lo, fmt))
    w_w, w_h = torch.randn(gc, gc, 1, k, generator=gen) / (gc * k) ** 0.5, torch.randn(gc, gc, k, 1, generator=gen) / (gc * k) ** 0.5
    b_w, b_h = 0.1 * torch.randn(gc, generator=gen), 0.1 * torch.randn(gc, generator=gen)
    blob = LF.pack_band_weights(w_w, w_h, products, fmt).to(device)
    bias = (LF.band_bias(b_w).to(device), LF.band_bias(b_h).to(device))
    p = LF.FigsrMixParams()
    p.batch, p.H, p.W, p.fmt, p.products, p.ksize, p.gc, p.planes, p.pass_planes = N, H, W, fmt, products, k, gc, planes, ps
    p.w_packed, p.bias_w, p.bias_h = blob.data_ptr(), bias[0].data_ptr(), bias[1].data_ptr()
    G.bind(p, 'g', 1)
    X.bind(p, 'x', 1)
    HWp.bind(p, 'hw', 1)
    # the float64 reference on what the kernel reads: hi + lo everywhere, but the hi halves alone for the band inputs in one product
    gr, xr, hr = _read(G, 1, planes), _read(X, 1, planes), _read(HWp, 1, P)
    xb = xr if products == 3 else X.hi[:, 1 : 1 + planes].double().permute(0, 1, 4, 2, 3).reshape(N, 8 * planes, H, W).cpu()
    c0 = 8 * ps + gc
    conv_w = F.conv2d(xb[:, c0 : c0 + gc], w_w.double(), b_w.double(), padding=(0, k // 2))
    conv_h = F.conv2d(xb[:, c0 + gc : c0 + 2 * gc], w_h.double(), b_h.double(), padding=(k // 2, 0))
    cat = torch.cat([xr[:, : 8 * ps], hr, conv_w, conv_h], 1)
    ref = F.silu(gr) * cat
    tol = (1e-5 if products == 3 else 2e-3) * max(conv_w.abs().max().item(), conv_h.abs().max().item())
    conv_bar = torch.zeros_like(ref)
    conv_bar[:, 8 * ps + gc :] = F.silu(gr[:, 8 * ps + gc :]).abs() * tol
    return p, ref, conv_bar, planes, dict(G=G, X=X, HW=HWp, w=(w_w, w_h), b=(b_w, b_h), keep=(blob, bias))


def _composition(device, case, p, planes, fmt, with_lo):
    """What rsa_figsr_mix replaces: each band embedded in a zero K x K kernel through rsa_plk_conv, then rsa_gfisr_gate over all planes."""
    H, W, k, gc, ps, P = p.H, p.W, p.ksize, p.gc, p.pass_planes, p.gc // 8
    X, HWp, G = case['X'], case['HW'], case['G']
    cat = Planes.empty(N, planes, H, W, device, with_lo, fmt)
    cat.hi[:, :ps] = X.hi[:, 1 : 1 + ps]
    cat.hi[:, ps : ps + P] = HWp.hi[:, 1 : 1 + P]
    if with_lo:
        cat.lo[:, :ps] = X.lo[:, 1 : 1 + ps]
        cat.lo[:, ps : ps + P] = HWp.lo[:, 1 : 1 + P]
    keep = []
    for band, (wt, bt) in enumerate(zip(case['w'], case['b'])):
        full = torch.zeros(gc, gc, k, k)
        if band == 0:
            full[:, :, k // 2, :] = wt[:, :, 0, :]
        else:
            full[:, :, :, k // 2] = wt[:, :, :, 0]
        blob, bias = plk.pack_plk_weights(full.to(device), p.products, fmt), plk.plk_bias(bt.to(device))
        a = 1 + ps + (1 + band) * P
        src = Planes(X.hi[:, a : a + P], None if X.lo is None else X.lo[:, a : a + P])
        plk.plk_conv(plk.plk_params(blob, bias, k, p.products, src, cat, ps + (1 + band) * P), ops.current_stream_ptr(device))
        keep += [blob, bias]
    gp = L.GatedDwConvParams()
    gp.batch, gp.H, gp.W, gp.fmt, gp.i_planes, gp.n_segments = N, H, W, fmt, planes, 0
    G.bind(gp, 'g', 1)
    cat.bind(gp, 'x')
    O = _buffer(N, planes, H, W, device, with_lo, fmt)
    O.bind(gp, 'out', 1)
    assert L.load().rsa_gfisr_gate(C.byref(gp), L.ACT_SILU, _stream(device)) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    return _read(O, 1, planes)


@pytest.mark.parametrize('hw,k,gc,ps,fmt,with_lo', CASES, ids=IDS)
def test_mix(device, hw, k, gc, ps, fmt, with_lo):
    p, ref, conv_bar, planes, case = _mix_case(device, hw, k, gc, ps, fmt, with_lo)
    before = [(t.hi.clone(), None if t.lo is None else t.lo.clone()) for t in (case['G'], case['X'], case['HW'])]
    O = _buffer(N, planes, *hw, device, with_lo, fmt)
    O.bind(p, 'out', 1)
    assert L.load().rsa_figsr_mix(C.byref(p), _stream(device)) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    _outside_untouched(O, 1, planes)
    for t, (hi, lo) in zip((case['G'], case['X'], case['HW']), before):  # the inputs are left alone
        assert torch.equal(t.hi, hi) and (lo is None or torch.equal(t.lo, lo))
    got = _read(O, 1, planes)
    assert torch.isfinite(got).all()
    plane_bar = _plane_bar(ref, fmt, with_lo)
    err = (got - ref).abs()
    bar = conv_bar + plane_bar
    print(f'MEASURE mix {hw[0]}x{hw[1]} k{k} gc{gc} pass{ps}: worst error {err.max().item():.3e}, worst error / bar {(err / bar).max().item():.3f}')
    assert (err <= bar).all()
    # the second check, against code that already exists
    comp = _composition(device, case, p, planes, fmt, with_lo)
    diff = (got - comp).abs()
    print(f'MEASURE mix against plk_conv + gate {hw[0]}x{hw[1]} k{k} gc{gc}: worst difference / (2 plane bars) {(diff / (2 * plane_bar)).max().item():.3f}')
    assert (diff <= 2 * plane_bar).all()


INPUT = [((6, 6), torch.float32, PF_BF16, True), ((7, 9), torch.float16, PF_F16, True), ((9, 6), torch.bfloat16, PF_BF16, True), ((8, 13), torch.float32, PF_F16, False),
         ((33, 70), torch.float32, PF_BF16, True), ((12, 7), torch.float16, PF_BF16, False)]  # fmt: skip


def _input(device, x, shift, scale, fmt, with_lo, override=None):
    n, c, h, w = x.shape
    H, W = h + 8 + h % 2, w + 8 + w % 2
    P = _buffer(n, 1, H, W, device, with_lo, fmt)
    keep = [x.to(device).contiguous(), shift.to(device), scale.to(device)]
    p = LF.FigsrInputParams()
    p.batch, p.C, p.src_h, p.src_w, p.pad, p.dtype, p.fmt = n, c, h, w, 4, ops.rsa_dtype(x.dtype), fmt
    p.x, p.shift, p.scale_norm = (t.data_ptr() for t in keep)
    P.bind(p, 'out', 1)
    for k, v in (override or {}).items():
        setattr(p, k, v)
    return L.load().rsa_figsr_input(C.byref(p), _stream(device)), P, keep


@pytest.mark.parametrize('hw,dtype,fmt,with_lo', INPUT, ids=[f'{h}x{w}-{str(d)[6:]}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for (h, w), d, f, lo in INPUT])
def test_input(device, hw, dtype, fmt, with_lo):
    h, w = hw
    gen = torch.Generator().manual_seed(3 * h + w)
    x = torch.rand(N, 3, h, w, generator=gen).to(dtype)
    shift, scale = torch.tensor([0.4, 0.5, 0.55]), torch.tensor([0.2, 1 / 6, 0.15])
    rc, P, _ = _input(device, x, shift, scale, fmt, with_lo)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    _outside_untouched(P, 1, 1)
    got = _read(P, 1, 1)
    v = (x.double() - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1)
    ref = F.pad(v, (4, 4 + w % 2, 4, 4 + h % 2), mode='reflect')
    assert got.shape[2:] == ref.shape[2:] and got.shape[2] % 2 == 0 and got.shape[3] % 2 == 0
    err = (got[:, :3] - ref).abs()
    bar = _plane_bar(ref, fmt, with_lo)
    print(f'MEASURE input {h}x{w} {dtype}: worst error {err.max().item():.3e}, worst error / bar {(err / bar).max().item():.3f}')
    assert (err <= bar).all()
    assert (got[:, 3:] == 0).all()  # the tail channels of the plane
    if dtype == torch.float32 and with_lo and fmt == PF_BF16:  # a true f32 division: hi + lo of bf16 keeps 16 bits of it
        f32 = F.pad((x - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1), (4, 4 + w % 2, 4, 4 + h % 2), mode='reflect').double()
        assert ((got[:, :3] - f32).abs() <= 2.0**-16 * f32.abs() + 1e-30).all()


OUTPUT = [((12, 14), (2, 3), (6, 8), torch.float32), ((28, 32), (8, 8), (12, 14), torch.float16), ((40, 36), (16, 16), (9, 7), torch.bfloat16), ((7, 70), (0, 0), (7, 70), torch.float32)]


def _output(device, y, shift, scale, origin, size, dtype, override=None):
    n, c, H, W = y.shape
    out = torch.full((n, c, *size), SENTINEL, dtype=dtype, device=device)
    keep = [y.to(device).contiguous(), shift.to(device), scale.to(device)]
    p = LF.FigsrOutputParams()
    p.batch, p.C, p.H, p.W, p.y0, p.x0, p.out_h, p.out_w, p.dtype = n, c, H, W, *origin, *size, ops.rsa_dtype(dtype)
    p.y, p.shift, p.scale_norm, p.out = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), out.data_ptr()
    for k, v in (override or {}).items():
        setattr(p, k, v)
    return L.load().rsa_figsr_output(C.byref(p), _stream(device)), out, keep


@pytest.mark.parametrize('full,origin,size,dtype', OUTPUT, ids=[f'{f[0]}x{f[1]}-{str(d)[6:]}' for f, _, _, d in OUTPUT])
def test_output(device, full, origin, size, dtype):
    gen = torch.Generator().manual_seed(full[0] + size[1])
    y = torch.randn(N, 3, *full, generator=gen)
    shift, scale = torch.tensor([0.4, 0.5, 0.55]), torch.tensor([0.2, 1 / 6, 0.15])
    rc, out, _ = _output(device, y, shift, scale, origin, size, dtype)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    win = y[:, :, origin[0] : origin[0] + size[0], origin[1] : origin[1] + size[1]]
    want = (win * scale.view(1, 3, 1, 1) + shift.view(1, 3, 1, 1)).to(dtype)  # a product and a sum in f32, rounded once to the dtype
    assert torch.equal(out.cpu(), want)


def test_error_codes(device):
    p, _, _, planes, case = _mix_case(device, (6, 8), 11, 8, 5, PF_BF16, True)
    O = _buffer(N, planes, 6, 8, device, True, PF_BF16)
    O.bind(p, 'out', 1)
    lib, stream = L.load(), _stream(device)

    def mix(**fields):
        q = LF.FigsrMixParams.from_buffer_copy(p)
        for k, v in fields.items():
            setattr(q, k, v)
        return lib.rsa_figsr_mix(C.byref(q), stream)

    assert mix() == 0
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(reserved0=1), dict(fmt=2), dict(products=2), dict(planes=7), dict(pass_planes=4), dict(pass_planes=-1),
               dict(w_packed=None), dict(bias_w=None), dict(bias_h=None), dict(g_hi=None), dict(x_hi=None), dict(x_lo=None), dict(hw_hi=None), dict(out_hi=None),
               dict(g_plane_stride=47), dict(x_plane_stride=47), dict(hw_plane_stride=47), dict(out_plane_stride=47), dict(out_hi=p.x_hi), dict(out_hi=p.g_hi)):  # fmt: skip
        assert mix(**kw) == E_ARG, kw
    for kw in (dict(ksize=12), dict(ksize=1), dict(ksize=33), dict(gc=4), dict(gc=24), dict(products=1), dict(fmt=PF_F16)):
        assert mix(**kw) == E_UNSUPPORTED, kw
    odd = torch.zeros(64, device=device).data_ptr() + 8
    for key in ('w_packed', 'bias_w', 'bias_h', 'g_hi', 'g_lo', 'x_hi', 'x_lo', 'hw_hi', 'hw_lo', 'out_hi', 'out_lo'):
        assert mix(**{key: odd}) == E_ALIGN, key
    assert lib.rsa_figsr_mix(None, stream) == E_ARG and lib.rsa_figsr_band_packed_weight_bytes(12, 8, 3) == -1

    x = torch.rand(N, 3, 6, 7)
    sh, sc = torch.full((3,), 0.5), torch.full((3,), 0.25)
    inp = lambda **fields: _input(device, x, sh, sc, PF_BF16, True, override=fields)[0]  # noqa: E731
    assert inp() == 0
    for kw in (dict(batch=0), dict(C=0), dict(src_h=0), dict(src_w=0), dict(reserved0=1), dict(pad=-1), dict(pad=6), dict(src_h=5), dict(dtype=L.U8), dict(fmt=2),
               dict(x=None), dict(shift=None), dict(scale_norm=None), dict(out_hi=None), dict(out_plane_stride=14 * 16 - 1)):  # fmt: skip
        assert inp(**kw) == E_ARG, kw
    assert inp(C=9) == E_UNSUPPORTED
    for key in ('out_hi', 'out_lo'):
        assert inp(**{key: odd}) == E_ALIGN, key
    assert lib.rsa_figsr_input(None, stream) == E_ARG

    y = torch.randn(N, 3, 12, 14)
    outp = lambda **fields: _output(device, y, sh, sc, (2, 3), (6, 8), torch.float32, override=fields)[0]  # noqa: E731
    assert outp() == 0
    for kw in (dict(batch=0), dict(C=0), dict(H=0), dict(W=0), dict(out_h=0), dict(out_w=0), dict(reserved0=1), dict(y0=-1), dict(x0=-1), dict(y0=7), dict(x0=7),
               dict(dtype=L.U8), dict(y=None), dict(shift=None), dict(scale_norm=None), dict(out=None)):  # fmt: skip
        assert outp(**kw) == E_ARG, kw
    assert lib.rsa_figsr_output(None, stream) == E_ARG
    torch.cuda.synchronize()
