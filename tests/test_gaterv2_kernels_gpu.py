"""Kernel-level parity of rsa_gaterv2_linear_attention (csrc/gaterv2.hip) through the C-ABI against float64 computed from the plane-rounded
inputs the kernels actually read (value = hi + lo, exact in f32 for both plane formats): every (C, m) and token count of the issue, batch 1
and 3, with and without lo planes in both plane formats, strides larger than the map, junk in the zero-padded q / k channels, bit-equal
repeats, sentinel-filled outputs and workspace tails.

The bar is a first-order forward-error bound derived here, per output element, from the kernels' operation counts and the magnitudes of the
f64 intermediates (u = 2^-24, the unit roundoff of f32; a chain of k fmas is within k u of the sum of the absolute values of its terms).
Nothing in it is fitted to what the kernel returns.  Cn = the number of 128-token chunks, N = H W tokens.

  |q|^2, |k|^2           an m-fma chain of non-negative terms: relative m u; the square root halves it and adds u, the reciprocal adds u,
                         the product with the channel adds u:           rel qn, kn <= (m / 2 + 3) u =: rk
  M_jc = sum_n kn_j v_c  a chain of at most 128 fmas per chunk, the chunks added in order:
                                                                        |d M_jc| <= (128 + Cn + rk / u) u sum_n |kn_j v_c| =: dM
  ksum_j                 likewise, and the addition of eps:             |d ksum_j| <= (128 + Cn + rk / u) u sum_n |kn_j| + u |ksum_j| =: dk
  vsum_c                                                                |d vsum_c| <= (128 + Cn) u sum_n |v_c| =: dv
  den = N + sum_j qn_j ksum_j   an m-fma chain and one addition (N is exact):
                                                                        |d den| <= sum_j |qn_j| dk_j + (m u + rk) sum_j |qn_j ksum_j| + u |den|
  t = 1 / den                                                           rel t <= |d den| / |den| + u =: rt
  num_c = vsum_c + sum_j qn_j M_jc   an m-fma chain from vsum_c:        |d num_c| <= dv_c + sum_j |qn_j| dM_jc + (m u + rk) (|vsum_c| + sum_j |qn_j M_jc|)
  out = num t            one product, then the planes' rounding:        |d out| <= |t| |d num| + |out| (rt + u) + e_fmt |out| + floor
  e_fmt = 2^-8 (bf16 hi), 2^-11 (fp16 hi), 2^-16 / 2^-22 with a lo plane (the residual is exact in f32 and rounded once more); floor = half
  an fp16 subnormal step, 2^-25, for fp16.

Conditioning, asserted on the f64 side: every q and k token vector has a norm of at least 0.25, and den >= N / 2.  The inputs are built so
that both hold (every |q|, |k| element is at least 0.25; channel j of q and of k carries one sign per image, so that every term of
qn . ksum is non-negative and den >= N whatever the token count), and
tests/test_gaterv2_capi.py checks the same construction on the CPU for every case here (the cases, the inputs and the reference are in
tests/gaterv2_attn_cases.py, which both read).
"""

import ctypes as C

import pytest
import torch

from gaterv2_attn_cases import CASES, EPS, FORMATS, make_inputs, reference
from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gaterv2 as LG2
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
BATCHES = (1, 3)


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _to_planes(x, fmt, with_lo, device):
    p = nchw_to_planes(x, with_lo, fmt)
    read = planes_to_nchw(p, x.shape[1]).double()
    return Planes(p.hi.to(device), None if p.lo is None else p.lo.to(device)), read


def _guarded_planes(n, planes, h, w, fmt, with_lo, device):
    """Output planes with a sentinel plane in front and one behind in every image (a batch stride larger than the planes)."""
    dt = torch.bfloat16 if fmt == PF_BF16 else torch.float16
    hi = torch.full((n, planes + 2, h, w, 8), SENTINEL, dtype=dt, device=device)
    lo = torch.full((n, planes + 2, h, w, 8), SENTINEL, dtype=dt, device=device) if with_lo else None
    return Planes(hi[:, 1 : planes + 1], None if lo is None else lo[:, 1 : planes + 1]), (hi, lo)


def _guards_intact(store, planes):
    return all(bool((t[:, 0] == SENTINEL).all()) and bool((t[:, planes + 1] == SENTINEL).all()) for t in store if t is not None)


def _run(device, c, m, qp: Planes, fmt, with_lo, strides=None):
    lib = L.load()
    b, h, w = qp.n, qp.h, qp.w
    out, store = _guarded_planes(b, c // 8, h, w, fmt, with_lo, device)
    nbytes = lib.rsa_gaterv2_attn_workspace_bytes(b, h, w, c, m)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=device)
    p = LG2.AttnParams()
    p.batch, p.H, p.W, p.C, p.m, p.fmt, p.eps = b, h, w, c, m, fmt, EPS
    qp.bind(p, 'qkv')
    if strides is not None:
        p.qkv_plane_stride, p.qkv_batch_stride = strides
    out.bind(p, 'out')
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
    assert lib.rsa_gaterv2_linear_attention(C.byref(p), _stream(device)) == 0, lib.rsa_last_error_string()
    torch.cuda.synchronize()
    return out, store, ws, nbytes


def _cpu(out: Planes, c):
    return planes_to_nchw(Planes(out.hi.cpu(), None if out.lo is None else out.lo.cpu()), c).double()


@pytest.mark.parametrize('c,m,hw', CASES, ids=[f'C{c}-m{m}-{h * w}' for c, m, (h, w) in CASES])
def test_linear_attention(device, c, m, hw):
    x3 = make_inputs(c, m, hw)
    worst = 0.0
    for batch in BATCHES:
        x = x3[:batch]
        for fmt, with_lo in FORMATS:
            qp, read = _to_planes(x, fmt, with_lo, device)
            ref, bar = reference(read, c, m, fmt, with_lo)
            out, store, ws, nbytes = _run(device, c, m, qp, fmt, with_lo)
            got = _cpu(out, c)
            assert torch.isfinite(got).all()
            ratio = ((got - ref).abs() / bar).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, f'batch {batch} fmt {fmt} lo {with_lo}: worst err / bound {ratio:.3f}'
            assert _guards_intact(store, c // 8) and bool((ws[nbytes // 4 :] == SENTINEL).all())
            out2, _, ws2, _ = _run(device, c, m, qp, fmt, with_lo)  # bit-equal reruns, the workspace included
            assert torch.equal(out2.hi, out.hi) and (out.lo is None or torch.equal(out2.lo, out.lo)) and torch.equal(ws2, ws)
    print(f'MEASURE rsa_gaterv2_linear_attention C {c} m {m} {hw[0] * hw[1]} tokens: worst err / bound {worst:.3f}')


@pytest.mark.parametrize('fmt,with_lo', FORMATS)
def test_the_padded_q_and_k_channels_change_no_bit(device, fmt, with_lo):
    """m = 6 in 8-channel planes: junk in channels 6 and 7 of the q and of the k plane of a copy gives the same bits."""
    c, m, hw = 96, 6, (3, 43)
    x = make_inputs(c, m, hw)
    junk = x.clone()
    gen = torch.Generator().manual_seed(5)
    junk[:, 6:8] = 50 * torch.randn(3, 2, *hw, generator=gen)
    junk[:, 14:16] = 50 * torch.randn(3, 2, *hw, generator=gen)
    junk[0, 6, 0, 0], junk[0, 15, 1, 2] = float('inf'), float('nan')
    a, _, _, _ = _run(device, c, m, _to_planes(x, fmt, with_lo, device)[0], fmt, with_lo)
    b, _, _, _ = _run(device, c, m, _to_planes(junk, fmt, with_lo, device)[0], fmt, with_lo)
    assert torch.equal(a.hi, b.hi) and (a.lo is None or torch.equal(a.lo, b.lo))
    assert torch.isfinite(_cpu(b, c)).all()


@pytest.mark.parametrize('fmt,with_lo', [(PF_BF16, True), (PF_F16, False)])
def test_plane_and_batch_strides_larger_than_the_map(device, fmt, with_lo):
    """The input planes with a row of sentinels under every plane and a plane of sentinels behind every image: the same bits as packed."""
    c, m, hw = 32, 2, (5, 27)
    h, w = hw
    x = make_inputs(c, m, hw)
    qp, _ = _to_planes(x, fmt, with_lo, device)
    want, _, _, _ = _run(device, c, m, qp, fmt, with_lo)
    planes = qp.planes

    def spread(t):
        big = torch.full((3, planes + 1, h + 1, w, 8), SENTINEL, dtype=t.dtype, device=device)
        big[:, :planes, :h] = t
        return big

    hi, lo = spread(qp.hi), None if qp.lo is None else spread(qp.lo)
    view = Planes(hi[:, :planes, :h], None if lo is None else lo[:, :planes, :h])
    got, store, _, _ = _run(device, c, m, view, fmt, with_lo, strides=((h + 1) * w, (planes + 1) * (h + 1) * w))
    assert torch.equal(got.hi, want.hi) and (want.lo is None or torch.equal(got.lo, want.lo)) and _guards_intact(store, c // 8)
