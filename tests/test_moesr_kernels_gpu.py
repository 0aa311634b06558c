"""Kernel-level parity of rsa_moesr_stream (csrc/moesr.hip): every mode x {LayerNorm planes, plain planes, no planes} x {stream written,
not written} over dim 8 / 40 / 64 / 128, maps 5x6, 7x70 (wider than one tile row) and 16x16, batch 2, both plane formats with and without
lo halves, the planes at an offset inside a larger sentinel-filled buffer (nothing outside the range is written), and every error code.

The map size of a case is the size of the SMALLER side of the launch: the stream itself in mode 0, the half-resolution output in mode 1
(the source is twice that), the half-resolution source in mode 2 (the stream is twice that).

Bars (the project's own):
  s_out in mode 1, and in mode 2 without s2_in   bit-equal to torch f32 (pixel_unshuffle; pixel_shuffle(a) + s)
  s_out in mode 0 and the three-term sum         1e-6 * max|ref| of an f64 reference
  planes with lo halves (LayerNorm or plain)     3e-5 * max|ref| of the f64 LayerNorm (or copy) of the kernel's own f32 s_out (test_swinir_gpu.py)
  planes without lo halves                       one unit of the format at each reference value's own magnitude, on top of the bar above:
                                                 the plane holds the rounding of the kernel's f32 value, and that value is only within
                                                 the f32 bar of the f64 reference -- an absolute distance that does not shrink with the
                                                 value, while the unit of a LayerNorm output near zero does (2^-27 at 1e-6 in bf16)
C is a multiple of 8, so a last plane has no tail channels to zero; the unused components of mode 1's last source group (dim 40: 10
channels in 3 groups) are NaN in the input and must not reach any output.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_moesr as LM
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
EPS = 1e-6
N = 2
CONFIGS = [  # dim, map, plane format, lo halves
    (8, (5, 6), PF_BF16, True), (40, (7, 70), PF_BF16, True), (64, (16, 16), PF_F16, True), (128, (5, 6), PF_F16, False),
    (40, (16, 16), PF_BF16, False), (128, (7, 70), PF_BF16, True), (64, (5, 6), PF_F16, True), (8, (7, 70), PF_F16, False),
]  # fmt: skip
OUTPUTS = [(planes, stream) for planes in ('ln', 'plain', None) for stream in (True, False) if planes or stream]
_inputs: dict = {}


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _to_map(x, nan_tail=False):
    m = nchw_to_f32map(x)
    if nan_tail and x.shape[1] % 4:
        m[:, -1, :, :, x.shape[1] % 4 :] = float('nan')
    return m


def inputs(mode, dim, hw):
    """The operands of a case (CPU, f32 NCHW) and the references they share: made once, never modified."""
    key = (mode, dim, hw)
    if key not in _inputs:
        gen = torch.Generator().manual_seed(1000 * mode + dim + 7 * hw[0] + hw[1])
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        h, w = hw
        H, W = (2 * h, 2 * w) if mode == 2 else (h, w)  # the output stream
        d = dict(H=H, W=W, gamma=1.0 + 0.25 * rnd(dim), ln_gamma=1.0 + 0.25 * rnd(dim), ln_beta=0.1 * rnd(dim))
        if mode == 0:
            d.update(a=rnd(N, dim, H, W), s_in=rnd(N, dim, H, W))
            d['ref'] = d['a'].double() * d['gamma'].double()[None, :, None, None] + d['s_in'].double()
        elif mode == 1:
            d.update(a=rnd(N, dim // 4, 2 * H, 2 * W))
            d['ref'] = F.pixel_unshuffle(d['a'], 2)  # f32: bit-equal
        else:
            d.update(a=rnd(N, 4 * dim, h, w), s_in=rnd(N, dim, H, W), s2_in=rnd(N, dim, H, W))
            d['ref'] = F.pixel_shuffle(d['a'], 2) + d['s_in']  # f32: bit-equal
            d['ref3'] = F.pixel_shuffle(d['a'], 2).double() + d['s_in'].double() + d['s2_in'].double()
        _inputs[key] = d
    return _inputs[key]


def _layer_norm(x, g, b):
    u = x.mean(1, keepdim=True)
    v = (x - u).pow(2).mean(1, keepdim=True)
    return g[None, :, None, None] * ((x - u) / torch.sqrt(v + EPS)) + b[None, :, None, None]


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


def _launch(device, mode, dim, d, *, planes, stream, fmt=PF_BF16, with_lo=True, s2=False, in_place=False, plane0=1, override=None):
    """Fill the descriptor from the case ``d`` and launch; returns (status, s_out map or None, plane buffer or None, tensors to keep)."""
    H, W = d['H'], d['W']
    dev = lambda t: t.to(device).contiguous()  # noqa: E731
    keep = {k: dev(d[k]) for k in ('gamma', 'ln_gamma', 'ln_beta')}
    keep['a'] = dev(_to_map(d['a'], nan_tail=True))
    for k in ('s_in', 's2_in'):
        if k in d:
            keep[k] = dev(_to_map(d[k]))
    p = LM.MoesrStreamParams()
    p.batch, p.H, p.W, p.C, p.mode, p.fmt = N, H, W, dim, mode, fmt
    p.a_H, p.a_W = d['a'].shape[2:]
    p.a = keep['a'].data_ptr()
    p.gamma = keep['gamma'].data_ptr() if mode == 0 else None
    p.s_in = keep['s_in'].data_ptr() if mode != 1 else None
    p.s2_in = keep['s2_in'].data_ptr() if s2 else None
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
        if planes == 'ln':
            p.ln_gamma, p.ln_beta, p.eps = keep['ln_gamma'].data_ptr(), keep['ln_beta'].data_ptr(), EPS
    for k, v in (override or {}).items():  # descriptor fields set last, whatever the case filled in
        setattr(p, k, v)
    rc = L.load().rsa_moesr_stream(C.byref(p), C.c_void_p(ops.current_stream_ptr(device)))
    return rc, s_out, P, keep


@pytest.mark.parametrize('planes,stream', OUTPUTS, ids=[f'{p or "noplanes"}-{"stream" if s else "nostream"}' for p, s in OUTPUTS])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('dim,hw,fmt,with_lo', CONFIGS, ids=[f'd{d}-{h}x{w}-{"f16" if f else "bf16"}-{"lo" if lo else "hi"}' for d, (h, w), f, lo in CONFIGS])
def test_every_mode_and_output_form(device, dim, hw, fmt, with_lo, mode, planes, stream):
    d = inputs(mode, dim, hw)
    rc, s_out, P, keep = _launch(device, mode, dim, d, planes=planes, stream=stream, fmt=fmt, with_lo=with_lo)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    ref = d['ref']
    s = ref.double()
    if stream:
        got = f32map_to_nchw(s_out.cpu(), dim)
        if mode == 0:
            err, bar = (got.double() - ref).abs().max().item(), 1e-6 * ref.abs().max().item()
            print(f'mode 0 s_out: {err:.3e} (bar {bar:.3e})')
            assert err <= bar
        else:
            assert torch.equal(got, ref)  # a permutation (+ one f32 add): bit-equal
        s = got.double()  # the planes are judged against the kernel's own stream
    if planes:
        pl = dim // 8
        want = _layer_norm(s, d['ln_gamma'].double(), d['ln_beta'].double()) if planes == 'ln' else s
        got = _read(P, 1, pl)
        assert torch.isfinite(got).all()
        if with_lo:
            err, bar = (got - want).abs().max().item(), 3e-5 * want.abs().max().item()
            print(f'mode {mode} {planes} planes: {err:.3e} (bar {bar:.3e})')
            assert err <= bar
        else:
            over = ((got - want).abs() - _unit(want, fmt)).max().item()
            bar = 3e-5 * want.abs().max().item()
            print(f'mode {mode} {planes} planes, hi only: worst error minus one unit {over:.3e} (bar {bar:.3e})')
            assert over <= bar
        for t in (P.hi, P.lo) if P.lo is not None else (P.hi,):  # nothing outside the plane range was written
            assert (t[:, :1] == SENTINEL).all() and (t[:, 1 + pl :] == SENTINEL).all()


@pytest.mark.parametrize('dim,hw', [(40, (5, 6)), (64, (7, 70))])
def test_mode2_three_term_sum(device, dim, hw):
    d = inputs(2, dim, hw)
    rc, s_out, P, keep = _launch(device, 2, dim, d, planes='plain', stream=True, s2=True)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got, ref = f32map_to_nchw(s_out.cpu(), dim), d['ref3']
    assert (got.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    assert torch.equal(got, (d['ref'] + d['s2_in']))  # and in the reference's order of additions: (up + x) + trunk
    assert (_read(P, 1, dim // 8) - got.double()).abs().max().item() <= 3e-5 * ref.abs().max().item()


@pytest.mark.parametrize('mode', [0, 2])
def test_stream_in_place(device, mode):
    """s_out == s_in, as the plan runs the block tails and the MSG exits."""
    d = inputs(mode, 40, (7, 70))
    rc, s_out, P, keep = _launch(device, mode, 40, d, planes='ln', stream=True, in_place=True)
    assert rc == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    got = f32map_to_nchw(s_out.cpu(), 40)
    if mode == 0:
        assert (got.double() - d['ref']).abs().max().item() <= 1e-6 * d['ref'].abs().max().item()
    else:
        assert torch.equal(got, d['ref'])
    want = _layer_norm(got.double(), d['ln_gamma'].double(), d['ln_beta'].double())
    assert (_read(P, 1, 5) - want).abs().max().item() <= 3e-5 * want.abs().max().item()


def test_error_codes(device):
    E_ARG, E_ALIGN = -1, -3

    def run(case_mode, d, planes='ln', stream=True, **fields):
        return _launch(device, case_mode, 8, d, planes=planes, stream=stream, override=fields)[0]

    d0, d1, d2 = (inputs(m, 8, (5, 6)) for m in (0, 1, 2))
    assert run(0, d0) == 0 and run(1, d1) == 0 and run(2, d2) == 0
    # geometry
    for kw in (dict(batch=0), dict(H=0), dict(W=0), dict(mode=3), dict(mode=-1), dict(reserved0=1), dict(fmt=2), dict(C=0), dict(C=12), dict(C=136), dict(C=4)):
        assert run(0, d0, **kw) == E_ARG, kw
    # the size of a: mode 0 reads it at H x W; an odd source size in mode 1 and an odd stream size in mode 2 are refused
    assert run(0, d0, a_H=6) == E_ARG
    assert run(1, d1, a_H=9) == E_ARG and run(1, d1, a_W=11) == E_ARG and run(1, d1, a_H=12) == E_ARG
    assert run(2, d2, H=9) == E_ARG and run(2, d2, W=11) == E_ARG and run(2, d2, a_H=4) == E_ARG
    # required pointers
    assert run(0, d0, a=None) == E_ARG and run(0, d0, gamma=None) == E_ARG and run(0, d0, s_in=None) == E_ARG and run(2, d2, s_in=None) == E_ARG
    assert run(0, d0, planes=None, stream=False) == E_ARG  # no output at all
    assert run(0, d0, out_hi=None) == E_ARG  # out_lo without out_hi
    assert run(0, d0, ln_beta=None) == E_ARG and run(0, d0, eps=0.0) == E_ARG
    assert run(0, d0, out_plane_stride=29) == E_ARG
    assert L.load().rsa_moesr_stream(None, None) == E_ARG
    # alignment: every pointer
    x = torch.zeros(64, device=device)
    odd = x.data_ptr() + 4
    for key in ('a', 'gamma', 's_in', 's_out', 'ln_gamma', 'ln_beta', 'out_hi', 'out_lo'):
        assert run(0, d0, **{key: odd}) == E_ALIGN, key
    assert run(2, d2, s2_in=odd) == E_ALIGN
    torch.cuda.synchronize()
