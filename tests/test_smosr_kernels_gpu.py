"""Kernel-level parity of csrc/smosr.hip against float64 computed by torch on the CPU from the exact values the device buffers hold.

rsa_smosr_gate   C 8 / 48 / 128, maps 3x4, 5x7 and 7x70 (wider than a wave), batch 2, both plane formats with and without lo halves, with and
                 without the stream, with and without s2_in, in place (s_out == s_in), the planes at an offset inside a sentinel-filled buffer.
                 Bars: the f32 stream within max(1e-6 * |ref|max, 4 x the error torch's own float32 evaluation of the formula shows against the
                 same float64) -- the first is test_moesr_kernels_gpu.py's, the second covers tanhf's few ulps and is measured on the
                 reference side; planes with lo halves within 3e-5 * |ref|max of the kernel's own stream (or of the f64 reference where no
                 stream is written); planes without lo halves one unit of the format on top (test_moesr_kernels_gpu.py).
rsa_smosr_pad    bit equality with F.pad(x, (2, 2, 2, 2), 'reflect') encoded by rsa_nchw_to_planes: 3x3, 3x8, 9x11; 1 and 3 channels.
rsa_smosr_pa     C 8 / 24 / 32 / 64 / 128, maps 3x5, 16x16, 17x67, batch 2, both formats, one and three products.  Bar: 4 x the error of the path
                 it replaces on the same inputs against the same float64 -- rsa_conv2d (1x1) to an f32 map in the same format and products,
                 then the gate and LeakyReLU in float32 torch.  Both errors are printed with a MEASURE prefix.
Both return their documented error codes on bad arguments, and rsa_check_status() is 0 after every test.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_smosr as LS
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map
from resselt_amd.engine.tensors import nchw_to_planes as planes_of

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
N = 2
E_ARG, E_ALIGN = -1, -3
_cache: dict = {}


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _unit(ref, fmt):
    """One unit of the plane format at the magnitude of ``ref`` (the spacing of its binade; the subnormal step near zero)."""
    mant, floor = (10, 2.0**-24) if fmt == PF_F16 else (7, 2.0**-133)
    _, e = torch.frexp(ref.abs())
    return torch.clamp(torch.ldexp(torch.ones_like(ref), e - 1 - mant), min=floor)


def _read(p: Planes, plane0, planes):
    v = p.hi[:, plane0 : plane0 + planes].double()
    if p.lo is not None:
        v = v + p.lo[:, plane0 : plane0 + planes].double()
    n, _, h, w, _ = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(n, 8 * planes, h, w).cpu()


# ---- rsa_smosr_gate --------------------------------------------------------------------------------------------------------------------
def gate_inputs(dim, hw):
    """Operands (CPU, f32 NCHW) and the references they share: made once, never modified."""
    key = ('gate', dim, hw)
    if key not in _cache:
        gen = torch.Generator().manual_seed(dim + 7 * hw[0] + hw[1])
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        d = dict(a=rnd(N, 2 * dim, *hw), s_in=rnd(N, dim, *hw), s2_in=rnd(N, dim, *hw))
        v, g = d['a'][:, :dim], d['a'][:, dim:]
        d['ref'] = (v.double() + d['s_in'].double()) * torch.tanh(g.double())
        d['ref2'] = d['ref'] + d['s2_in'].double()
        f32 = (v + d['s_in']) * torch.tanh(g)
        d['f32_err'] = (f32.double() - d['ref']).abs().max().item()  # what float32 torch itself shows against the same float64
        d['f32_err2'] = ((f32 + d['s2_in']).double() - d['ref2']).abs().max().item()
        _cache[key] = d
    return _cache[key]


def gate_launch(device, dim, hw, d, *, planes, stream, fmt=PF_BF16, with_lo=True, s2=False, in_place=False, plane0=1, override=None, alias_s2=False):
    H, W = hw
    dev = lambda t: nchw_to_f32map(t).to(device).contiguous()  # noqa: E731
    keep = {k: dev(d[k]) for k in ('a', 's_in', 's2_in')}
    p = LS.SmosrGateParams()
    p.batch, p.H, p.W, p.C, p.fmt = N, H, W, dim, fmt
    p.a, p.s_in = keep['a'].data_ptr(), keep['s_in'].data_ptr()
    p.s2_in = keep['s_in'].data_ptr() if alias_s2 else keep['s2_in'].data_ptr() if s2 else None
    s_out = None
    if stream:
        s_out = keep['s_in'] if in_place else torch.full((N, dim // 4, H, W, 4), SENTINEL, device=device)
        p.s_out = s_out.data_ptr()
    P = None
    if planes:
        P = Planes.empty(N, dim // 8 + plane0 + 2, H, W, device, with_lo, fmt)
        P.hi.fill_(SENTINEL)
        if P.lo is not None:
            P.lo.fill_(SENTINEL)
        P.bind(p, 'out', plane0)
    for k, v in (override or {}).items():
        setattr(p, k, v)
    rc = L.load().rsa_smosr_gate(C.byref(p), C.c_void_p(ops.current_stream_ptr(device)))
    return rc, s_out, P, keep


def gate_check(d, dim, fmt, with_lo, s_out, P, s2, what):
    ref = d['ref2'] if s2 else d['ref']
    s = ref
    if s_out is not None:
        got = f32map_to_nchw(s_out.cpu(), dim)
        err = (got.double() - ref).abs().max().item()
        bar = max(1e-6 * ref.abs().max().item(), 4 * (d['f32_err2'] if s2 else d['f32_err']))
        print(f'MEASURE gate {what} s_out: {err:.3e} (bar {bar:.3e}; float32 torch {d["f32_err2"] if s2 else d["f32_err"]:.3e})')
        assert err <= bar
        s = got.double()
    if P is not None:
        pl = dim // 8
        got = _read(P, 1, pl)
        assert torch.isfinite(got).all()
        bar = 3e-5 * s.abs().max().item()
        over = ((got - s).abs() - (0 if with_lo else _unit(s, fmt))).max().item()
        print(f'MEASURE gate {what} planes{"" if with_lo else ", hi only (minus one unit)"}: {over:.3e} (bar {bar:.3e})')
        assert over <= bar
        for t in (P.hi, P.lo) if P.lo is not None else (P.hi,):  # nothing outside the plane range was written
            assert (t[:, :1] == SENTINEL).all() and (t[:, 1 + pl :] == SENTINEL).all()


# dim, map, plane format, lo halves: the full product
GATE_CONFIGS = [(c, hw, fmt, lo) for c in (8, 48, 128) for hw in ((3, 4), (5, 7), (7, 70)) for fmt in (PF_BF16, PF_F16) for lo in (True, False)]
GATE_OUTPUTS = [(planes, stream) for planes in (True, False) for stream in (True, False) if planes or stream]


@pytest.mark.parametrize('s2', [False, True], ids=['', 'trunk'])
@pytest.mark.parametrize('planes,stream', GATE_OUTPUTS, ids=[f'{"planes" if p else "noplanes"}-{"stream" if s else "nostream"}' for p, s in GATE_OUTPUTS])
@pytest.mark.parametrize('dim,hw,fmt,with_lo', GATE_CONFIGS, ids=[f'c{d}-{h}x{w}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for d, (h, w), f, lo in GATE_CONFIGS])
def test_gate_every_output_form(device, dim, hw, fmt, with_lo, planes, stream, s2):
    d = gate_inputs(dim, hw)
    rc, s_out, P, keep = gate_launch(device, dim, hw, d, planes=planes, stream=stream, fmt=fmt, with_lo=with_lo, s2=s2)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    gate_check(d, dim, fmt, with_lo, s_out, P, s2, f'c{dim} {hw}')


@pytest.mark.parametrize('s2', [False, True], ids=['', 'trunk'])
@pytest.mark.parametrize('dim,hw', [(48, (7, 70)), (128, (5, 7)), (8, (3, 4))])
def test_gate_in_place(device, dim, hw, s2):
    """s_out == s_in, as the plan runs every block but the two that open a new stream."""
    d = gate_inputs(dim, hw)
    rc, s_out, P, keep = gate_launch(device, dim, hw, d, planes=True, stream=True, s2=s2, in_place=True)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    assert s_out is keep['s_in']
    gate_check(d, dim, PF_BF16, True, s_out, P, s2, f'in place c{dim} {hw}')


def test_gate_trunk_aliasing_the_stream(device):
    """s_in == s2_in (blocks_2 of one block: the shortcut and the trunk residual are the same map)."""
    d = dict(gate_inputs(48, (5, 7)))
    d['s2_in'] = d['s_in']
    v, g = d['a'][:, :48], d['a'][:, 48:]
    d['ref2'] = (v.double() + d['s_in'].double()) * torch.tanh(g.double()) + d['s_in'].double()
    d['f32_err2'] = ((((v + d['s_in']) * torch.tanh(g)) + d['s_in']).double() - d['ref2']).abs().max().item()
    rc, s_out, P, keep = gate_launch(device, 48, (5, 7), d, planes=True, stream=True, s2=True, alias_s2=True)
    assert rc == 0
    torch.cuda.synchronize()
    gate_check(d, 48, PF_BF16, True, s_out, P, True, 'trunk == shortcut')


def test_gate_error_codes(device):
    d = gate_inputs(8, (3, 4))

    def run(planes=True, stream=True, **fields):
        return gate_launch(device, 8, (3, 4), d, planes=planes, stream=stream, override=fields)[0]

    assert run() == 0
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(reserved0=1), dict(fmt=2), dict(C=0), dict(C=12), dict(C=136), dict(C=4)):
        assert run(**kw) == E_ARG, kw
    assert run(a=None) == E_ARG and run(s_in=None) == E_ARG
    assert run(planes=False, stream=False) == E_ARG  # no output at all
    assert run(out_hi=None) == E_ARG  # out_lo without out_hi
    assert run(out_plane_stride=11) == E_ARG
    assert L.load().rsa_smosr_gate(None, None) == E_ARG
    a = nchw_to_f32map(d['a']).to(device)
    assert run(a=a.data_ptr(), s_out=a.data_ptr()) == E_ARG  # in place on a: the two maps have different batch strides
    odd = torch.zeros(64, device=device).data_ptr() + 4
    for key in ('a', 's_in', 's2_in', 's_out', 'out_hi', 'out_lo'):
        assert run(**{key: odd}) == E_ALIGN, key
    torch.cuda.synchronize()


# ---- rsa_smosr_pad ---------------------------------------------------------------------------------------------------------------------
def _pad_launch(device, src, out: Planes, fields=None):
    p = LS.SmosrPadParams()
    n, c, h, w = src.shape
    p.batch, p.C, p.src_h, p.src_w, p.pad, p.dtype, p.fmt = n, c, h, w, 2, ops.rsa_dtype(src.dtype), out.fmt
    p.x = src.data_ptr()
    out.bind(p, 'out')
    for k, v in (fields or {}).items():
        setattr(p, k, v)
    return L.load().rsa_smosr_pad(C.byref(p), C.c_void_p(ops.current_stream_ptr(device)))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
@pytest.mark.parametrize('fmt,with_lo', [(PF_BF16, True), (PF_F16, True), (PF_F16, False)], ids=['bf16-lo', 'f16-lo', 'f16-hi'])
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('hw', [(3, 3), (3, 8), (9, 11)])
def test_pad_is_bit_equal_to_pad_then_nchw_to_planes(device, hw, c, fmt, with_lo, dtype):
    gen = torch.Generator().manual_seed(11 * hw[0] + hw[1] + c)
    x = torch.rand(N, c, *hw, generator=gen).to(dtype).to(device)
    H, W = hw[0] + 4, hw[1] + 4
    want = Planes.empty(N, 1, H, W, device, with_lo, fmt)
    ops.nchw_to_planes(F.pad(x, (2, 2, 2, 2), 'reflect').contiguous(), want)
    got = Planes.empty(N, 1, H, W, device, with_lo, fmt)
    got.hi.fill_(SENTINEL)
    assert _pad_launch(device, x, got) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(got.hi.view(torch.int16), want.hi.view(torch.int16))
    if with_lo:
        assert torch.equal(got.lo.view(torch.int16), want.lo.view(torch.int16))
    assert (got.hi[..., c:] == 0).all()  # tail channels are written as zero


def test_pad_error_codes(device):
    x = torch.rand(N, 3, 3, 5, device=device)
    out = Planes.empty(N, 1, 7, 9, device, True, PF_BF16)
    run = lambda **kw: _pad_launch(device, x, out, fields=kw)  # noqa: E731
    assert run() == 0
    for kw in (dict(batch=0), dict(C=0), dict(src_h=0), dict(src_w=0), dict(reserved0=1), dict(pad=-1), dict(pad=3), dict(dtype=L.U8), dict(dtype=7), dict(fmt=2),
               dict(x=None), dict(out_hi=None), dict(out_plane_stride=62)):  # fmt: skip
        assert run(**kw) == E_ARG, kw
    odd = torch.zeros(64, device=device).data_ptr() + 4
    assert run(out_hi=odd) == E_ALIGN and run(out_lo=odd) == E_ALIGN
    assert L.load().rsa_smosr_pad(None, None) == E_ARG
    torch.cuda.synchronize()


# ---- rsa_smosr_pa ----------------------------------------------------------------------------------------------------------------------
class _Prec(int):
    """What ``ConvWeights.from_oihw`` reads of the module's ``Prec``: the products (the int) and the plane format."""

    def __new__(cls, products, fmt):
        obj = super().__new__(cls, products)
        obj.fmt = fmt
        return obj


def pa_inputs(c, hw):
    key = ('pa', c, hw)
    if key not in _cache:
        gen = torch.Generator().manual_seed(3 * c + 5 * hw[0] + hw[1])
        x = torch.randn(N, c, *hw, generator=gen)
        w = torch.randn(c, c, generator=gen) * (1.5 / c**0.5)  # z = W x + b of order 1: the sigmoid works, neither flat nor linear
        b = torch.randn(c, generator=gen) * 0.5
        _cache[key] = dict(x=x, w=w, b=b)
    return _cache[key]


def pa_reference(xv, w, b):
    """float64 from the values the input planes hold (``xv``) and the f32 weights."""
    z = torch.einsum('oi,nihw->nohw', w.double(), xv) + b.double()[None, :, None, None]
    return F.leaky_relu(xv * torch.sigmoid(z), 0.2)


def _pa_launch(device, c, x_pl: Planes, out: Planes, wf, bias, nprod, plane0=0, fields=None):
    p = LS.SmosrPaParams()
    p.batch, p.H, p.W, p.C, p.fmt, p.products, p.slope = x_pl.n, x_pl.h, x_pl.w, c, x_pl.fmt, nprod, 0.2
    p.w_frag, p.bias = wf.data_ptr(), bias.data_ptr()
    x_pl.bind(p, 'in')
    out.bind(p, 'out', plane0)
    for k, v in (fields or {}).items():
        setattr(p, k, v)
    return L.load().rsa_smosr_pa(C.byref(p), C.c_void_p(ops.current_stream_ptr(device)))


def _to_device(pl: Planes, device) -> Planes:
    return Planes(pl.hi.to(device), None if pl.lo is None else pl.lo.to(device))


PA_CONFIGS = [(c, hw) for c in (8, 24, 32, 64, 128) for hw in ((3, 5), (16, 16), (17, 67))]  # the full product


@pytest.mark.parametrize('products', [1, 3])
@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('c,hw', PA_CONFIGS, ids=[f'c{c}-{h}x{w}' for c, (h, w) in PA_CONFIGS])
def test_pa_against_the_path_it_replaces(device, c, hw, fmt, products):
    """Input and output planes carry lo halves in both modes (one product multiplies the hi halves alone, as rsa_conv2d does; the gate
    reads hi + lo in both paths), so the comparison is between two f32-accurate stores of the same formula."""
    d = pa_inputs(c, hw)
    H, W = hw
    x_pl = _to_device(planes_of(d['x'], True, fmt), device)
    xv = _read(x_pl, 0, (c + 7) // 8)[:, :c]  # f64 of what the planes hold
    ref = pa_reference(xv, d['w'], d['b'])
    # the path it replaces: rsa_conv2d (1x1) to an f32 map in the same format and products, the gate and LeakyReLU in float32 torch
    cw = ops.ConvWeights.from_oihw(d['w'][:, :, None, None].to(device), d['b'].to(device), _Prec(products, fmt), device=device)
    zmap = torch.empty((N, (c + 3) // 4, H, W, 4), dtype=torch.float32, device=device)
    ops.run_convs([ops.conv_params(cw, x_pl, H, W, out_f32=zmap)], device)
    torch.cuda.synchronize()
    z32 = f32map_to_nchw(zmap.cpu(), c)
    alt = F.leaky_relu(xv.float() * torch.sigmoid(z32), 0.2)
    alt_err = (alt.double() - ref).abs().max().item()
    # the fused kernel, into planes 1.. of a sentinel-filled buffer
    wf, bias = LS.pack_pa_weights(d['w'], d['b'], products, fmt, device)
    out = Planes.empty(N, c // 8 + 3, H, W, device, True, fmt)
    out.hi.fill_(SENTINEL)
    out.lo.fill_(SENTINEL)
    assert _pa_launch(device, c, x_pl, out, wf, bias, products, plane0=1) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = _read(out, 1, c // 8)
    err = (got - ref).abs().max().item()
    print(f'MEASURE pa c{c} {H}x{W} {"f16" if fmt else "bf16"} x{products}: fused {err:.3e}  conv + f32 torch {alt_err:.3e}  (bar {4 * alt_err:.3e}; |ref|max {ref.abs().max():.3f})')
    assert torch.isfinite(got).all() and err <= 4 * alt_err
    for t in (out.hi, out.lo):
        assert (t[:, :1] == SENTINEL).all() and (t[:, 1 + c // 8 :] == SENTINEL).all()


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('c,hw', [(32, (17, 67)), (24, (3, 5))])
def test_pa_hi_only_planes(device, c, hw, fmt):
    """One product on planes without lo halves, as the one-product policy runs it: the result is the rounding of an f32 value that is
    within the bar above of the reference -- one unit of the format on top."""
    d = pa_inputs(c, hw)
    H, W = hw
    x_pl = _to_device(planes_of(d['x'], False, fmt), device)
    xv = _read(x_pl, 0, (c + 7) // 8)[:, :c]
    ref = pa_reference(xv, d['w'], d['b'])
    cw = ops.ConvWeights.from_oihw(d['w'][:, :, None, None].to(device), d['b'].to(device), _Prec(1, fmt), device=device)
    zmap = torch.empty((N, (c + 3) // 4, H, W, 4), dtype=torch.float32, device=device)
    ops.run_convs([ops.conv_params(cw, x_pl, H, W, out_f32=zmap)], device)
    torch.cuda.synchronize()
    alt = F.leaky_relu(xv.float() * torch.sigmoid(f32map_to_nchw(zmap.cpu(), c)), 0.2)
    alt_err = (alt.double() - ref).abs().max().item()
    wf, bias = LS.pack_pa_weights(d['w'], d['b'], 1, fmt, device)
    out = Planes.empty(N, c // 8, H, W, device, False, fmt)
    assert _pa_launch(device, c, x_pl, out, wf, bias, 1) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = _read(out, 0, c // 8)
    over = ((got - ref).abs() - _unit(ref, fmt)).max().item()
    print(f'MEASURE pa hi-only c{c} {H}x{W} {"f16" if fmt else "bf16"}: worst error minus one unit {over:.3e} (bar {4 * alt_err:.3e})')
    assert over <= 4 * alt_err


def test_pa_in_place(device):
    d = pa_inputs(64, (16, 16))
    x_pl = _to_device(planes_of(d['x'], True, PF_BF16), device)
    ref = pa_reference(_read(x_pl, 0, 8), d['w'], d['b'])
    wf, bias = LS.pack_pa_weights(d['w'], d['b'], 3, PF_BF16, device)
    assert _pa_launch(device, 64, x_pl, x_pl, wf, bias, 3) == 0
    torch.cuda.synchronize()
    assert (_read(x_pl, 0, 8) - ref).abs().max().item() <= 3e-5 * ref.abs().max().item()


def test_pa_error_codes(device):
    d = pa_inputs(8, (3, 5))
    x_pl = _to_device(planes_of(d['x'], True, PF_BF16), device)
    out = Planes.empty(N, 1, 3, 5, device, True, PF_BF16)
    wf, bias = LS.pack_pa_weights(d['w'], d['b'], 3, PF_BF16, device)
    run = lambda **kw: _pa_launch(device, 8, x_pl, out, wf, bias, 3, fields=kw)  # noqa: E731
    assert run() == 0
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(reserved0=1), dict(fmt=2), dict(C=0), dict(C=12), dict(C=136), dict(products=2), dict(products=0),
               dict(w_frag=None), dict(bias=None), dict(in_hi=None), dict(out_hi=None), dict(in_lo=None), dict(in_plane_stride=14), dict(out_plane_stride=14)):  # fmt: skip
        assert run(**kw) == E_ARG, kw
    # in place where it is illegal: the same hi buffer with another stride, or with another lo buffer
    assert run(out_hi=x_pl.hi_ptr(), out_lo=x_pl.lo_ptr(), out_plane_stride=16) == E_ARG
    assert run(out_hi=x_pl.hi_ptr()) == E_ARG
    odd = torch.zeros(64, device=device).data_ptr() + 4
    for key in ('w_frag', 'bias', 'in_hi', 'in_lo', 'out_hi', 'out_lo'):
        assert run(**{key: odd}) == E_ALIGN, key
    assert L.load().rsa_smosr_pa(None, None) == E_ARG
    torch.cuda.synchronize()
