"""Kernel-level parity of rsa_gated_dwconv and rsa_bilinear_add (csrc/mosr.hip) against f64 CPU references:
every compiled tap shape and both bands, an identity segment, both plane formats with and without lo halves, ragged maps, batch 2,
strided plane ranges inside larger buffers (a sentinel proves nothing outside the output range is written), and the error codes."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes

pytestmark = pytest.mark.gpu

SENTINEL = 3.0


def _planes(n, planes, h, w, device, fmt, with_lo):
    p = Planes.empty(n, planes, h, w, device, with_lo, fmt)
    p.hi.fill_(SENTINEL)
    if p.lo is not None:
        p.lo.fill_(SENTINEL)
    return p


def _read(p: Planes, plane0, planes):
    """Planes [plane0, plane0 + planes) as f64 NCHW (hi + lo)."""
    v = p.hi[:, plane0 : plane0 + planes].double()
    if p.lo is not None:
        v = v + p.lo[:, plane0 : plane0 + planes].double()
    n, _, h, w, _ = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(n, 8 * planes, h, w).cpu()


def _write(p: Planes, plane0, x):
    """f32 NCHW (8 * planes channels) into planes [plane0, ...) as hi (+ lo) in the buffer's format."""
    n, c, h, w = x.shape
    v = x.reshape(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).to(p.hi.device)
    hi = v.to(p.hi.dtype)
    p.hi[:, plane0 : plane0 + c // 8] = hi
    if p.lo is not None:
        p.lo[:, plane0 : plane0 + c // 8] = (v - hi.float()).to(p.lo.dtype)


def _params(n, h, w, fmt, i_planes, segs, G, g0, X, x0, O, o0):
    p = L.GatedDwConvParams()
    p.batch, p.H, p.W, p.fmt, p.i_planes, p.n_segments = n, h, w, fmt, i_planes, len(segs)
    keep = []
    for s, (pl, kh, kw, wt, bt) in enumerate(segs):
        p.seg[s].planes, p.seg[s].kh, p.seg[s].kw = pl, kh, kw
        if wt is not None:
            wt, bt = wt.float().contiguous().to(G.hi.device), bt.float().contiguous().to(G.hi.device)
            keep += [wt, bt]
            p.seg[s].weight, p.seg[s].bias = wt.data_ptr(), bt.data_ptr()
    p.g_hi, p.g_lo, p.g_plane_stride, p.g_batch_stride = G.hi_ptr(g0), G.lo_ptr(g0), G.plane_stride, G.batch_stride
    p.x_hi, p.x_lo, p.x_plane_stride, p.x_batch_stride = X.hi_ptr(x0), X.lo_ptr(x0), X.plane_stride, X.batch_stride
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = O.hi_ptr(o0), O.lo_ptr(o0), O.plane_stride, O.batch_stride
    return p, keep


def _run(p, device):
    return L.load().rsa_gated_dwconv(C.byref(p), C.c_void_p(ops.current_stream_ptr(device)))


def _reference(g, x, i_planes, segs):
    parts = [x[:, : 8 * i_planes]]
    c0 = 8 * i_planes
    for pl, kh, kw, wt, bt in segs:
        xs = x[:, c0 : c0 + 8 * pl]
        if (kh, kw) == (1, 1):
            parts.append(xs)
        else:
            parts.append(F.conv2d(xs, wt.double().reshape(8 * pl, 1, kh, kw), bt.double(), padding=(kh // 2, kw // 2), groups=8 * pl))
        c0 += 8 * pl
    return F.mish(g) * torch.cat(parts, 1)


def _case(device, n, h, w, fmt, with_lo, i_planes, shapes, seed=0, extra=(2, 1, 3)):
    """Random g / x / weights; g, x and out live at plane offsets inside larger buffers of their own."""
    gen = torch.Generator().manual_seed(seed)
    segs = []
    for pl, kh, kw in shapes:
        if (kh, kw) == (1, 1):
            segs.append((pl, 1, 1, None, None))
        else:
            segs.append((pl, kh, kw, torch.randn(8 * pl, kh * kw, generator=gen) / (kh * kw) ** 0.5, torch.randn(8 * pl, generator=gen) * 0.1))
    P = i_planes + sum(s[0] for s in shapes)
    g0, x0, o0 = extra
    G = _planes(n, P + g0 + 1, h, w, device, fmt, with_lo)
    X = _planes(n, P + x0 + 2, h, w, device, fmt, with_lo)
    O = _planes(n, P + o0 + 1, h, w, device, fmt, with_lo)
    _write(G, g0, torch.randn(n, 8 * P, h, w, generator=gen))
    _write(X, x0, torch.randn(n, 8 * P, h, w, generator=gen))
    p, keep = _params(n, h, w, fmt, i_planes, segs, G, g0, X, x0, O, o0)
    assert _run(p, device) == 0, L.load().rsa_last_error_string()
    torch.cuda.synchronize()
    ref = _reference(_read(G, g0, P), _read(X, x0, P), i_planes, segs)
    got = _read(O, o0, P)
    tol = (2e-5 if with_lo else 1e-2) * max(1.0, ref.abs().max().item()) * (8 if fmt == PF_F16 and not with_lo else 1)
    err = (got - ref).abs().max().item()
    assert err <= tol, f'max-abs {err:.3e} > {tol:.3e}'
    # nothing outside the output plane range was written
    for t in (O.hi, O.lo) if O.lo is not None else (O.hi,):
        assert (t[:, :o0] == SENTINEL).all() and (t[:, o0 + P :] == SENTINEL).all()
    return keep


@pytest.mark.parametrize('k', [3, 5, 7, 9, 11])
@pytest.mark.parametrize('band', ['square', 'row', 'col'])
def test_every_compiled_shape(device, k, band):
    kh, kw = {'square': (k, k), 'row': (1, k), 'col': (k, 1)}[band]
    _case(device, 1, 37, 45, PF_BF16, True, 1, [(2, kh, kw)], seed=k)


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
@pytest.mark.parametrize('with_lo', [True, False])
def test_formats_and_mosrv2_layout(device, fmt, with_lo):
    # passthrough planes, an identity segment, then 3x3, 1x11 and 11x1: four segments
    _case(device, 2, 33, 47, fmt, with_lo, 2, [(1, 1, 1), (1, 3, 3), (1, 1, 11), (1, 11, 1)], seed=3)


@pytest.mark.parametrize('hw', [(1, 1), (5, 4), (2, 9), (33, 47), (70, 31)])
def test_ragged_maps(device, hw):
    _case(device, 2, hw[0], hw[1], PF_BF16, True, 1, [(1, 7, 7), (1, 1, 11)], seed=hw[0] * 100 + hw[1])


def test_no_passthrough_and_wide_segments(device):
    _case(device, 1, 20, 64, PF_F16, True, 0, [(3, 5, 5), (2, 9, 1)], seed=11, extra=(0, 0, 0))


def test_error_codes(device):
    G = _planes(1, 4, 8, 8, device, PF_BF16, True)
    w = torch.zeros(8, 49, device=device)
    b = torch.zeros(8, device=device)

    def rc(**kw):
        segs = kw.pop('segs', [(1, 7, 7, w, b)])
        p, _ = _params(1, 8, 8, PF_BF16, 1, [], G, 0, G, 0, G, 2)
        p.n_segments = len(segs)
        for s, (pl, kh, kw_, wt, bt) in enumerate(segs):
            p.seg[s].planes, p.seg[s].kh, p.seg[s].kw = pl, kh, kw_
            p.seg[s].weight, p.seg[s].bias = (wt.data_ptr() if wt is not None else None), (bt.data_ptr() if bt is not None else None)
        for k, v in kw.items():
            setattr(p, k, v)
        return _run(p, device)

    assert rc() == 0
    for bad in ((1, 4, 4), (1, 13, 13), (1, 3, 5), (1, 2, 1), (1, 1, 13)):
        assert rc(segs=[(*bad, w, b)]) == -2  # RSA_E_UNSUPPORTED
    assert rc(segs=[(1, 7, 7, None, None)]) == -1
    assert rc(segs=[(0, 7, 7, w, b)]) == -1
    assert rc(H=0) == -1 and rc(batch=0) == -1 and rc(fmt=2) == -1 and rc(n_segments=5) == -1
    assert rc(g_hi=None) == -1 and rc(out_hi=None) == -1
    assert rc(x_hi=G.hi_ptr() + 2) == -3 and rc(out_lo=G.lo_ptr() + 8) == -3  # RSA_E_ALIGN
    assert L.load().rsa_gated_dwconv(None, None) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize('scale', [1, 2, 3, 4])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_bilinear_add(device, scale, dtype):
    gen = torch.Generator().manual_seed(scale)
    n, c, h, w = 2, 3, 11, 13
    pad = 4 // scale if scale < 3 else 1
    ph, pw = h + (pad - h % pad) % pad, w + (pad - w % pad) % pad
    x = torch.rand(n, c, h, w, generator=gen)
    base = torch.randn(n, c, ph * scale, pw * scale, generator=gen)
    xp = F.pad(x.double(), (0, pw - w, 0, ph - h), 'reflect') if (ph > h or pw > w) else x.double()
    ref = base.double() + F.interpolate(xp, scale_factor=scale, mode='bilinear', align_corners=False)
    xd, out = x.to(device, dtype), base.to(device, dtype)
    p = L.BilinearAddParams()
    p.batch, p.C, p.h, p.w, p.pad_h, p.pad_w, p.scale, p.dtype = n, c, h, w, ph, pw, scale, ops.rsa_dtype(dtype)
    p.out_H, p.out_W, p.out_h, p.out_w = ph * scale, pw * scale, h * scale, w * scale  # the crop: only that region is written
    p.x, p.out = xd.data_ptr(), out.data_ptr()
    assert L.load().rsa_bilinear_add(C.byref(p), C.c_void_p(ops.current_stream_ptr(device))) == 0
    torch.cuda.synchronize()
    got = out.double().cpu()
    tol = 2e-6 if dtype == torch.float32 else 4e-3
    crop = (slice(None), slice(None), slice(0, h * scale), slice(0, w * scale))
    assert (got[crop] - ref[crop]).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
    assert torch.equal(out.cpu()[:, :, h * scale :], base.to(dtype)[:, :, h * scale :])
    p.pad_h = 2 * h
    assert L.load().rsa_bilinear_add(C.byref(p), C.c_void_p(ops.current_stream_ptr(device))) == -1
    p.pad_h, p.dtype = ph, L.U8
    assert L.load().rsa_bilinear_add(C.byref(p), C.c_void_p(ops.current_stream_ptr(device))) == -2
