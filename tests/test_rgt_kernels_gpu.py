"""Kernel-level GPU parity of csrc/rgt.hip against fp32 torch: rsa_rg_attention (every token against a pooled key / value set),
rsa_rg_reduce (t-fold 4x4 stride-4 depthwise reduction), rsa_layernorm_gelu, rsa_scale_add, and their error codes.

Tolerances: attention 1e-4 * scale with three products, 3e-2 with one fp16 product (as test_rect_attention_kernel); the elementwise
kernels 3e-5 * scale.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops, tensors

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -2  # RSA_E_ARG, RSA_E_UNSUPPORTED


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _q16(x):
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _head_pad(t, heads, d):
    """[n, heads*d, h, w] -> [n, heads*32, h, w] with zero pads."""
    n, _, h, w = t.shape
    out = torch.zeros((n, heads, 32, h, w))
    out[:, :, :d] = t.reshape(n, heads, d, h, w)
    return out.reshape(n, heads * 32, h, w)


def _planes(t, device, fmt):
    if fmt == 'f16':
        return tensors.nchw_to_planes(t.to(device), fmt=tensors.PF_F16)
    return tensors.nchw_to_planes(t.to(device))


def _attn_params(n, H, W, heads, nk, dq, dv, q, k, v, out, products, fmt):
    ap = L.RgAttnParams()
    ap.batch, ap.H, ap.W, ap.heads, ap.nkeys, ap.dim_qk, ap.dim_v, ap.products, ap.fmt = n, H, W, heads, nk, dq, dv, products, fmt
    ap.q_hi, ap.q_lo, ap.q_plane_stride, ap.q_batch_stride = q.hi_ptr(), q.lo_ptr(), q.plane_stride, q.batch_stride
    ap.k_hi, ap.k_lo, ap.k_plane_stride, ap.k_batch_stride = k.hi_ptr(), k.lo_ptr(), k.plane_stride, k.batch_stride
    ap.v_hi, ap.v_lo, ap.v_plane_stride, ap.v_batch_stride = v.hi_ptr(), v.lo_ptr(), v.plane_stride, v.batch_stride
    ap.out_hi, ap.out_lo, ap.out_plane_stride, ap.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    return ap


@pytest.mark.parametrize('mode', ['bf16x3', 'f16'])
# big: channel 0 of every q and k is set to `big`, which shifts every score by big^2 exactly (256: exp() of an unshifted score overflows)
@pytest.mark.parametrize('nk,heads,dq,dv,n,H,W,big', [
    (1, 2, 15, 30, 1, 17, 23, 0.0), (7, 3, 15, 30, 2, 9, 40, 0.0), (33, 6, 15, 30, 1, 31, 33, 0.0), (480, 2, 32, 32, 2, 20, 30, 0.0),
    (1024, 1, 8, 16, 1, 64, 50, 0.0), (3969, 2, 15, 30, 1, 16, 37, 0.0), (1024, 2, 32, 32, 1, 24, 24, 16.0),
])  # fmt: skip
def test_rg_attention_kernel(device, mode, nk, heads, dq, dv, n, H, W, big):
    kh, kw = (nk, 1) if nk < 64 else (nk // 32, 32) if nk % 32 == 0 else (63, 63)
    assert kh * kw == nk
    q = _rand((n, heads, H * W, dq), 1, 1.5)
    k = _rand((n, heads, nk, dq), 2, 1.5)
    if big:
        q[..., 0], k[..., 0] = big, big
    v = _rand((n, heads, nk, dv), 3, 1.0)
    if mode == 'bf16x3':
        q, k, v = _q16(q), _q16(k), _q16(v)
    else:
        q, k, v = q.half().float(), k.half().float(), v.half().float()
    ref = torch.softmax(q @ k.transpose(-1, -2), -1) @ v  # [n, heads, HW, dv]

    def img(t, h, w, d):
        return _head_pad(t.permute(0, 1, 3, 2).reshape(n, heads * d, h, w), heads, d)

    fmt = L.PF_F16 if mode == 'f16' else L.PF_BF16
    qp, kp, vp = (_planes(img(t, h, w, d), device, mode) for t, h, w, d in ((q, H, W, dq), (k, kh, kw, dq), (v, kh, kw, dv)))
    if mode == 'f16':
        qp, kp, vp = (tensors.Planes(p.hi, None) for p in (qp, kp, vp))
    out = tensors.Planes.empty(n, heads * 4, H, W, device, with_lo=mode == 'bf16x3', fmt=fmt)
    ap = _attn_params(n, H, W, heads, nk, dq, dv, qp, kp, vp, out, 3 if mode == 'bf16x3' else 1, fmt)
    L.check(L.load().rsa_rg_attention(C.byref(ap), _stream(device)), 'rsa_rg_attention')
    torch.cuda.synchronize()
    got = tensors.planes_to_nchw(out, heads * 32).cpu().reshape(n, heads, 32, H * W)
    assert dv == 32 or got[:, :, dv:].abs().max().item() == 0.0
    got = got[:, :, :dv].permute(0, 1, 3, 2)
    err = (got - ref).abs().max().item()
    tol = (1e-4 if mode == 'bf16x3' else 3e-2) * max(1.0, ref.abs().max().item())
    assert err <= tol, f'max-abs {err:.3e}'


def test_rg_attention_errors(device):
    n, H, W, heads = 1, 8, 8, 1
    q = tensors.Planes.empty(n, 4, H, W, device)
    kv = tensors.Planes.empty(n, 4, 4, 4, device)
    out = tensors.Planes.empty(n, 4, H, W, device)
    lib = L.load()

    def rc(**kw):
        ap = _attn_params(n, H, W, heads, 16, 15, 30, q, kv, kv, out, 3, L.PF_BF16)
        for k, v in kw.items():
            setattr(ap, k, v)
        return lib.rsa_rg_attention(C.byref(ap), _stream(device))

    assert rc() == 0
    assert rc(nkeys=0) == E_ARG
    assert rc(nkeys=3970) == E_ARG
    assert rc(dim_qk=33) == E_UNSUPPORTED
    assert rc(dim_v=40) == E_UNSUPPORTED
    assert rc(q_hi=None) == E_ARG
    assert rc(k_lo=None) == E_ARG
    assert rc(products=2) == E_UNSUPPORTED
    assert rc(k_plane_stride=8) == E_ARG
    assert lib.rsa_rg_attention(None, _stream(device)) == E_ARG
    torch.cuda.synchronize()


def _reduce_ref(x, w, b, t):
    for _ in range(t):
        x = F.conv2d(x, w, b, stride=4, groups=x.shape[1])
    return x


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16', 'f16'])
@pytest.mark.parametrize('t,n,c,H,W', [(1, 1, 8, 9, 13), (2, 2, 24, 35, 50), (3, 1, 16, 64, 200), (4, 1, 8, 259, 300)])
def test_rg_reduce_kernel(device, mode, t, n, c, H, W):
    x = _rand((n, c, H, W), 11, 2.0)
    w = (1 + 8 * _rand((c, 1, 4, 4), 12, 1 / 16)) / 16
    b = _rand((c,), 13, 0.1)
    if mode == 'f16':
        xq = x.half().float()
        xq = xq + (x - xq).half().float()
    else:
        xq = _q16(x) if mode == 'bf16x3' else x.bfloat16().float()
    ref = _reduce_ref(xq, w, b, t)
    fmt = L.PF_F16 if mode == 'f16' else L.PF_BF16
    xp = _planes(x, device, mode)
    if mode == 'bf16':
        xp = tensors.Planes(xp.hi, None)
    oh, ow = H >> (2 * t), W >> (2 * t)
    out = tensors.Planes.empty(n, c // 8, oh, ow, device, fmt=fmt)
    keep = [w.reshape(c, 16).contiguous().to(device), b.to(device)]
    rp = L.RgReduceParams()
    rp.batch, rp.H, rp.W, rp.planes, rp.times, rp.fmt = n, H, W, c // 8, t, fmt
    rp.in_hi, rp.in_lo, rp.in_plane_stride, rp.in_batch_stride = xp.hi_ptr(), xp.lo_ptr(), xp.plane_stride, xp.batch_stride
    rp.weight, rp.bias = keep[0].data_ptr(), keep[1].data_ptr()
    rp.out_hi, rp.out_lo, rp.out_plane_stride, rp.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    lib = L.load()
    L.check(lib.rsa_rg_reduce(C.byref(rp), _stream(device)), 'rsa_rg_reduce')
    torch.cuda.synchronize()
    got = tensors.planes_to_nchw(out, c).cpu()
    assert got.shape == ref.shape
    err = (got - ref).abs().max().item()
    assert err <= 3e-5 * max(1.0, ref.abs().max().item()), f'max-abs {err:.3e}'
    rp.times = 7
    assert lib.rsa_rg_reduce(C.byref(rp), _stream(device)) == E_UNSUPPORTED
    rp.times, rp.H = t, (1 << (2 * t)) - 1
    assert lib.rsa_rg_reduce(C.byref(rp), _stream(device)) == E_ARG
    torch.cuda.synchronize()


def test_layernorm_gelu_and_scale_add(device):
    n, c, h, w = 2, 36, 7, 9
    x = _rand((n, c, h, w), 21, 3.0)
    g, b = 1 + _rand((c,), 22, 0.3), _rand((c,), 23, 0.2)
    ref = F.gelu(F.layer_norm(x.permute(0, 2, 3, 1), (c,), g, b, 1e-5)).permute(0, 3, 1, 2)
    xm = tensors.nchw_to_f32map(x.to(device))
    out = tensors.Planes.empty(n, (c + 7) // 8, h, w, device)
    keep = [g.to(device), b.to(device)]
    lp = L.LayerNormParams()
    lp.batch, lp.H, lp.W, lp.C, lp.eps = n, h, w, c, 1e-5
    lp.x_f32, lp.gamma, lp.beta = xm.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr()
    lp.out_hi, lp.out_lo, lp.out_plane_stride, lp.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.check(L.load().rsa_layernorm_gelu(C.byref(lp), _stream(device)), 'rsa_layernorm_gelu')
    torch.cuda.synchronize()
    err = (tensors.planes_to_nchw(out, c).cpu() - ref).abs().max().item()
    assert err <= 3e-5 * max(1.0, ref.abs().max().item())
    # HAI: out += gamma * res on f32 maps
    r = _rand((n, c, h, w), 24, 2.0)
    o = _rand((n, c, h, w), 25, 2.0)
    rm, om = tensors.nchw_to_f32map(r.to(device)), tensors.nchw_to_f32map(o.to(device))
    L.check(L.load().rsa_scale_add(rm.data_ptr(), keep[0].data_ptr(), om.data_ptr(), n, h, w, c, _stream(device)), 'rsa_scale_add')
    torch.cuda.synchronize()
    err = (tensors.f32map_to_nchw(om, c).cpu() - (o + r * g[None, :, None, None])).abs().max().item()
    assert err <= 1e-6 * 8
