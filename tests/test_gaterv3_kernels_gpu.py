"""Kernel-level parity of GateRV3's entry points (csrc/gaterv3.hip) against float64 computed from the plane-rounded inputs the kernels
actually read (value = hi + lo, exact in f32 for both plane formats), rsa_gaterv3_shortcut bit for bit against torch, bit-equal repeats,
sentinel-filled outputs, and every error code with real device buffers.

The bars are first-order forward-error bounds derived here, per output element, from the kernels' operation counts and the magnitudes of the
f64 intermediates (u = 2^-24, the unit roundoff of f32; a chain of k fmas is within k u of the sum of the absolute values of its terms).
Nothing in them is fitted to what a kernel returns.

rsa_gaterv3_local_gate
  conv_o = b_o + 18 taps   an 18-fma chain from the bias:        |d conv_o| <= 18 u (|b_o| + sum_18 |w x|)
  s_c = conv_c conv_{dim+c}   one product:                       |d s_c| <= |conv_{dim+c}| |d conv_c| + |conv_c| |d conv_{dim+c}| + u |s_c| =: ds
  the planes               RNE to the format (8 significant bits in bf16, 11 in fp16), e_fmt = 2^-8 (bf16 hi), 2^-11 (fp16 hi), 2^-16 / 2^-22 with a lo plane (the residual is exact
                           in f32 and rounded once more), and half an fp16 subnormal step, 2^-25, for fp16:
                                                                 |d plane| <= ds + e_fmt |s_c| + floor
  a tile sum               the f32 s before the plane rounding; every value passes six additions of the wave butterfly and at most three
                           across the four waves:                |d sum| <= sum_tile ds + 9 u sum_tile |s|
rsa_gaterv3_sca_apply (fed by the launch above: a "chunked sum of length H W" in T tiles)
  mean_c = (sum of T tile sums) / HW   at most T additions on the way of any tile sum (runs of tiles, then the run sums) and a division:
                                                                 |d mean_c| <= (sum_px ds + (9 + T) u sum_px |s|) / HW + u |mean_c|
  a_o = gamma0_o (b_o + sum_c W_oc mean_c)   a dim-fma chain from the bias and a product:
                                    |d a_o| <= |gamma0_o| (sum_c |W_oc| |d mean_c| + (dim + 1) u (|b_o| + sum_c |W_oc mean_c|)) + u |a_o|
  out = s a + short        one fma on the s the kernel reads back from its planes (the reference uses those very planes):
                                                                 |d out| <= |s| |d a_o| + u |out|
rsa_gaterv3_channel_attention   (Cn chunks of 128 tokens, d = head_dim, T_h the temperature)
  G_ij, |q_i|^2, |k_j|^2   a 128-fma chain per chunk, the chunks added in order:   |d G_ij| <= (128 + Cn) u sum_t |q_i k_j| =: dG,
                           and relative (128 + Cn) u for the squared norms, half of it plus u for their square roots: rn
  l_ij = T_h G_ij / (|q_i| |k_j|)   two products and a division: |d l_ij| <= |T_h| dG / (|q_i| |k_j|) + |l_ij| (2 rn + 3 u) =: dl
  e_ij = exp(l_ij - m_i)   a subtraction, then expf within 2 ulp; an argument error becomes a relative one:
                                                                 rel e_ij <= dl_ij + max_j dl_ij + u |l_ij - m_i| + 2 u =: re_ij
  A_ij = e_ij / sum_j e_ij   d sequential additions and a division: |d A_ij| <= A_ij (re_ij + max_j re_ij + (d + 1) u) =: dA
  out_i = sum_j A_ij v_j   a d-fma chain:                          |d out_i| <= sum_j dA_ij |v_j| + d u sum_j A_ij |v_j|, then the planes' rounding
  Conditioning, asserted on the f64 side: every q and k row has an rms of at least 0.25 (so 1e-12 never binds and dG / (|q| |k|) stays of
  the order of (128 + Cn) u), and |l| <= |T_h| <= 5 by Cauchy-Schwarz, so the softmax inputs span at most 10.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import lib_gaterv3 as LG3
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
N = 2
U = 2.0**-24
E_ARG, E_UNSUPPORTED, E_ALIGN = -1, -2, -3
FORMATS = [(PF_BF16, True), (PF_BF16, False), (PF_F16, True), (PF_F16, False)]
HWS = [(1, 1), (1, 2), (2, 1), (3, 5), (8, 5), (7, 36), (33, 9), (64, 25)]  # the issue's list
CHUNK_HWS = [(7, 31), (8, 32), (9, 33), (17, 65)]  # one below, at and one above the 8 x 32 reduction tile; above two tiles on either axis
LOCAL_CASES = [(d, hw) for d in (8, 16) for hw in HWS + CHUNK_HWS] + [(d, hw) for d in (32, 128) for hw in [(1, 1), (7, 36), (33, 9), (64, 25), (9, 33)]]
ATTN_TOKENS = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (1, 127), (3, 43), (13, 79)]  # 1, 2, 63, 64, 65, chunk - 1, chunk + 1, 1027
ATTN_CASES = [(d, t) for d in (1, 2, 4, 8) for t in ATTN_TOKENS] + [(d, t) for d in (32, 64) for t in [(1, 1), (7, 9), (3, 43), (13, 79)]]


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _fmt_eps(fmt, with_lo):
    e = {(PF_BF16, False): 2.0**-8, (PF_F16, False): 2.0**-11, (PF_BF16, True): 2.0**-16, (PF_F16, True): 2.0**-22}[(fmt, with_lo)]
    return e, (2.0**-25 if fmt == PF_F16 else 0.0)


def _to_planes(x, fmt, with_lo, device):
    """x [N, C, H, W] f32 -> (device planes, the f64 value the kernel reads)."""
    p = nchw_to_planes(x, with_lo, fmt)
    read = planes_to_nchw(p, x.shape[1]).double()
    return Planes(p.hi.to(device), None if p.lo is None else p.lo.to(device)), read


def _guarded_planes(n, planes, h, w, fmt, with_lo, device):
    """Output planes with a sentinel plane in front and one behind in every image."""
    dt = torch.bfloat16 if fmt == PF_BF16 else torch.float16
    hi = torch.full((n, planes + 2, h, w, 8), SENTINEL, dtype=dt, device=device)
    lo = torch.full((n, planes + 2, h, w, 8), SENTINEL, dtype=dt, device=device) if with_lo else None
    return Planes(hi[:, 1 : planes + 1], None if lo is None else lo[:, 1 : planes + 1]), (hi, lo)


def _guards_intact(store, planes):
    return all(bool((t[:, 0] == SENTINEL).all()) and bool((t[:, planes + 1] == SENTINEL).all()) for t in store if t is not None)


def _record(name, ratio):
    print(f'MEASURE {name}: worst err / bound {ratio:.3f}')


# ------------------------------------------------------------------------------------------------------------------ local gate + sca
def _local_inputs(dim, hw, gen):
    x = torch.randn(N, 2 * dim, *hw, generator=gen)
    x[1] = x[1] * 1.7 + 0.6  # other statistics in the second image: a mean leaking across images shows
    w = torch.randn(2 * dim, 2, 3, 3, generator=gen) / 18**0.5
    b = 0.2 * torch.randn(2 * dim, generator=gen)
    sca_w = torch.randn(dim, dim, generator=gen) / dim**0.5
    sca_b = 0.3 * torch.randn(dim, generator=gen)
    gamma0 = torch.randn(dim, generator=gen)
    short = torch.randn(N, dim, *hw, generator=gen)
    return x, w, b, sca_w, sca_b, gamma0, short


def _local_reference(xr, w, b, dim):
    conv = F.conv2d(xr, w.double(), b.double(), padding=1, groups=dim)
    mag = F.conv2d(xr.abs(), w.double().abs(), b.double().abs(), padding=1, groups=dim)
    dconv = 18 * U * mag
    a, c = conv[:, :dim], conv[:, dim:]
    s = a * c
    ds = c.abs() * dconv[:, :dim] + a.abs() * dconv[:, dim:] + U * s.abs()
    return s, ds


def _tile_sums(t, hw):
    """[N, C, H, W] -> [N, tiles, C]: the sums over the 8 x 32 tiles in row-major tile order."""
    H, W = hw
    rows = []
    for y0 in range(0, H, LG3.TILE_H):
        for x0 in range(0, W, LG3.TILE_W):
            rows.append(t[:, :, y0 : y0 + LG3.TILE_H, x0 : x0 + LG3.TILE_W].sum((2, 3)))
    return torch.stack(rows, 1)


def _run_local(device, dim, hw, fmt, with_lo, tensors):
    x, w, b, sca_w, sca_b, gamma0, short = tensors
    H, W = hw
    lib = L.load()
    xp, xr = _to_planes(x, fmt, with_lo, device)
    out, store = _guarded_planes(N, dim // 8, H, W, fmt, with_lo, device)
    nbytes = lib.rsa_gaterv3_local_workspace_bytes(N, H, W, dim)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=device)
    keep = [t.to(device).contiguous() for t in (w.reshape(2 * dim, 18), b, sca_w, sca_b, gamma0, nchw_to_f32map(short))]
    p = LG3.LocalGateParams()
    p.batch, p.H, p.W, p.dim, p.fmt = N, H, W, dim, fmt
    xp.bind(p, 'x')
    out.bind(p, 'out')
    p.weight, p.bias, p.workspace, p.workspace_bytes = keep[0].data_ptr(), keep[1].data_ptr(), ws.data_ptr(), nbytes
    assert lib.rsa_gaterv3_local_gate(C.byref(p), _stream(device)) == 0, lib.rsa_last_error_string()
    omap = torch.full((N + 2, dim // 4, H, W, 4), SENTINEL, device=device)
    q = LG3.ScaApplyParams()
    q.batch, q.H, q.W, q.dim, q.fmt = N, H, W, dim, fmt
    out.bind(q, 's')
    q.sca_w, q.sca_b, q.gamma0, q.short_f32, q.out_f32 = keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), omap[1].data_ptr()
    q.workspace, q.workspace_bytes = ws.data_ptr(), nbytes
    assert lib.rsa_gaterv3_sca_apply(C.byref(q), _stream(device)) == 0, lib.rsa_last_error_string()
    torch.cuda.synchronize()
    return xr, out, store, ws, omap, nbytes


@pytest.mark.parametrize('dim,hw', LOCAL_CASES, ids=[f'd{d}-{h}x{w}' for d, (h, w) in LOCAL_CASES])
def test_local_gate_and_sca_apply(device, dim, hw):
    gen = torch.Generator().manual_seed(100 * dim + 7 * hw[0] + hw[1])
    tensors = _local_inputs(dim, hw, gen)
    x, w, b, sca_w, sca_b, gamma0, short = tensors
    H, W = hw
    tiles = -(-H // LG3.TILE_H) * -(-W // LG3.TILE_W)
    worst = [0.0, 0.0, 0.0]
    for fmt, with_lo in FORMATS:
        xr, out, store, ws, omap, nbytes = _run_local(device, dim, hw, fmt, with_lo, tensors)
        s, ds = _local_reference(xr, w, b, dim)
        e_fmt, floor = _fmt_eps(fmt, with_lo)
        # 1. the planes of s
        got_s = planes_to_nchw(Planes(out.hi.cpu(), None if out.lo is None else out.lo.cpu()), dim).double()
        bar = ds + e_fmt * s.abs() + floor
        worst[0] = max(worst[0], ((got_s - s).abs() / bar).max().item())
        assert ((got_s - s).abs() <= bar).all()
        assert _guards_intact(store, dim // 8)
        # 2. the tile sums
        part = ws[: N * tiles * dim].cpu().double().reshape(N, tiles, dim)
        ref_p, bar_p = _tile_sums(s, hw), _tile_sums(ds + 9 * U * s.abs(), hw)
        worst[1] = max(worst[1], ((part - ref_p).abs() / bar_p).max().item())
        assert ((part - ref_p).abs() <= bar_p).all()
        assert bool((ws[nbytes // 4 :] == SENTINEL).all())  # nothing behind the workspace
        # 3. s * a + short on the stream map, from the s the kernel reads back
        HW = H * W
        mean = s.sum((2, 3)) / HW
        dmean = (ds.sum((2, 3)) + (9 + tiles) * U * s.abs().sum((2, 3))) / HW + U * mean.abs()
        Wd, g0 = sca_w.double(), gamma0.double()
        lin = mean @ Wd.T + sca_b.double()
        a = g0 * lin
        da = g0.abs() * (dmean @ Wd.abs().T + (dim + 1) * U * (sca_b.double().abs() + mean.abs() @ Wd.abs().T)) + U * a.abs()
        ref_o = got_s * a[:, :, None, None] + short.double()
        bar_o = got_s.abs() * da[:, :, None, None] + U * ref_o.abs()
        got_o = f32map_to_nchw(omap[1 : N + 1].cpu(), dim).double()
        worst[2] = max(worst[2], ((got_o - ref_o).abs() / bar_o).max().item())
        assert ((got_o - ref_o).abs() <= bar_o).all()
        assert bool((omap[0] == SENTINEL).all()) and bool((omap[N + 1] == SENTINEL).all())
        # a second run: bit-equal planes, sums and map
        _, out2, _, ws2, omap2, _ = _run_local(device, dim, hw, fmt, with_lo, tensors)
        assert torch.equal(out2.hi, out.hi) and (out.lo is None or torch.equal(out2.lo, out.lo))
        assert torch.equal(ws2[: nbytes // 4], ws[: nbytes // 4]) and torch.equal(omap2, omap)
    _record(f'rsa_gaterv3_local_gate planes d{dim} {H}x{W}', worst[0])
    _record(f'rsa_gaterv3_local_gate tile sums d{dim} {H}x{W}', worst[1])
    _record(f'rsa_gaterv3_sca_apply d{dim} {H}x{W}', worst[2])


def test_the_mean_of_one_image_does_not_reach_the_other(device):
    dim, hw = 16, (9, 33)
    gen = torch.Generator().manual_seed(5)
    tensors = _local_inputs(dim, hw, gen)
    _, _, _, _, omap, _ = _run_local(device, dim, hw, PF_BF16, True, tensors)
    swapped = [t.flip(0).contiguous() if t.dim() == 4 and t.shape[0] == N and i in (0, 6) else t for i, t in enumerate(tensors)]
    _, _, _, _, omap_s, _ = _run_local(device, dim, hw, PF_BF16, True, swapped)
    assert torch.equal(omap[1], omap_s[2]) and torch.equal(omap[2], omap_s[1]) and not torch.equal(omap[1], omap[2])


# ------------------------------------------------------------------------------------------------------------------ attention
def _attn_inputs(d, hw, gen):
    Cc = 16 * d
    sign = lambda t: torch.where(t < 0, -1.0, 1.0)  # noqa: E731
    r = torch.randn(N, 3 * Cc, *hw, generator=gen)
    qkv = sign(r) * (0.25 + r.abs())  # every value at least 0.25 in magnitude: every row's rms is
    qkv[1] = qkv[1] * 1.5
    temp = torch.tensor([5.0, -3.0, 0.5, -0.25, 2.0, 1.0, -5.0, 4.0, 0.75, -1.5, 3.0, 0.1, -0.6, 1.25, 2.5, -2.0])
    return qkv, temp


def _attn_reference(qr, temp, d, hw, fmt, with_lo, heads=16):
    Cc, T = heads * d, hw[0] * hw[1]
    chunks = -(-T // LG3.TOKEN_CHUNK)
    q, k, v = (t.reshape(N, heads, d, T) for t in qr.split(Cc, 1))
    Th = temp.double().view(1, heads, 1, 1)
    G = q @ k.transpose(2, 3)
    dG = (128 + chunks) * U * (q.abs() @ k.abs().transpose(2, 3))
    nq, nk = q.norm(dim=3), k.norm(dim=3)
    assert (nq / T**0.5 >= 0.25).all() and (nk / T**0.5 >= 0.25).all()  # well conditioned rows: 1e-12 never binds
    rn = (128 + chunks) * U / 2 + U
    den = nq[..., :, None] * nk[..., None, :]
    l = Th * G / den
    assert (l.abs() <= Th.abs() * (1 + 1e-12)).all() and l.abs().max() <= 5.0 + 1e-9  # Cauchy-Schwarz: the softmax inputs span at most 10
    dl = Th.abs() * dG / den + l.abs() * (2 * rn + 3 * U)
    m = l.amax(3, keepdim=True)
    re = dl + dl.amax(3, keepdim=True) + U * (l - m).abs() + 2 * U
    A = torch.softmax(l, 3)
    dA = A * (re + re.amax(3, keepdim=True) + (d + 1) * U)
    out = A @ v
    dout = dA @ v.abs() + d * U * (A @ v.abs())
    e_fmt, floor = _fmt_eps(fmt, with_lo)
    return out.reshape(N, Cc, *hw), (dout + e_fmt * out.abs() + floor).reshape(N, Cc, *hw)


def _run_attn(device, d, hw, fmt, with_lo, qkv, temp):
    H, W = hw
    Cc = 16 * d
    lib = L.load()
    qp, qr = _to_planes(qkv, fmt, with_lo, device)
    out, store = _guarded_planes(N, Cc // 8, H, W, fmt, with_lo, device)
    nbytes = lib.rsa_gaterv3_attn_workspace_bytes(N, H, W, 16, d)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 8,), SENTINEL, device=device)
    t_dev = temp.to(device)
    p = LG3.AttnParams()
    p.batch, p.H, p.W, p.C, p.heads, p.head_dim, p.fmt = N, H, W, Cc, 16, d, fmt
    qp.bind(p, 'qkv')
    out.bind(p, 'out')
    p.temperature, p.workspace, p.workspace_bytes = t_dev.data_ptr(), ws.data_ptr(), nbytes
    assert lib.rsa_gaterv3_channel_attention(C.byref(p), _stream(device)) == 0, lib.rsa_last_error_string()
    torch.cuda.synchronize()
    return qr, out, store, ws, nbytes


@pytest.mark.parametrize('d,hw', ATTN_CASES, ids=[f'hd{d}-{h * w}' for d, (h, w) in ATTN_CASES])
def test_channel_attention(device, d, hw):
    gen = torch.Generator().manual_seed(1000 * d + 7 * hw[0] + hw[1])
    qkv, temp = _attn_inputs(d, hw, gen)
    worst = 0.0
    for fmt, with_lo in FORMATS:
        qr, out, store, ws, nbytes = _run_attn(device, d, hw, fmt, with_lo, qkv, temp)
        ref, bar = _attn_reference(qr, temp, d, hw, fmt, with_lo)
        got = planes_to_nchw(Planes(out.hi.cpu(), None if out.lo is None else out.lo.cpu()), 16 * d).double()
        worst = max(worst, ((got - ref).abs() / bar).max().item())
        assert ((got - ref).abs() <= bar).all(), f'worst err / bound {((got - ref).abs() / bar).max().item():.3f}'
        assert _guards_intact(store, 16 * d // 8) and bool((ws[nbytes // 4 :] == SENTINEL).all())
        _, out2, _, ws2, _ = _run_attn(device, d, hw, fmt, with_lo, qkv, temp)
        assert torch.equal(out2.hi, out.hi) and (out.lo is None or torch.equal(out2.lo, out.lo)) and torch.equal(ws2, ws)
    _record(f'rsa_gaterv3_channel_attention hd{d} {hw[0] * hw[1]} tokens', worst)


def test_fewer_heads_than_sixteen(device):
    """heads 4 x head_dim 6 = 24 channels: heads that straddle planes at another head count (the reference formula on [N, 4, 6, T])."""
    hw, heads, d = (5, 13), 4, 6
    gen = torch.Generator().manual_seed(11)
    r = torch.randn(N, 3 * heads * d, *hw, generator=gen)
    qkv = torch.where(r < 0, -1.0, 1.0) * (0.25 + r.abs())
    temp = torch.tensor([2.0, -1.0, 0.5, 4.0])
    lib = L.load()
    qp, qr = _to_planes(qkv, PF_BF16, True, device)
    out, store = _guarded_planes(N, 3, *hw, PF_BF16, True, device)
    nbytes = lib.rsa_gaterv3_attn_workspace_bytes(N, *hw, heads, d)
    ws = torch.empty(nbytes // 4, device=device)
    t_dev = temp.to(device)
    p = LG3.AttnParams()
    p.batch, p.H, p.W, p.C, p.heads, p.head_dim, p.fmt = N, hw[0], hw[1], heads * d, heads, d, PF_BF16
    qp.bind(p, 'qkv')
    out.bind(p, 'out')
    p.temperature, p.workspace, p.workspace_bytes = t_dev.data_ptr(), ws.data_ptr(), nbytes
    assert lib.rsa_gaterv3_channel_attention(C.byref(p), _stream(device)) == 0
    torch.cuda.synchronize()
    ref, bar = _attn_reference(qr, temp, d, hw, PF_BF16, True, heads=heads)
    q, k, v = (t.reshape(N, heads, d, -1) for t in qr.split(heads * d, 1))
    a = torch.softmax(F.normalize(q, dim=3) @ F.normalize(k, dim=3).transpose(2, 3) * temp.double().view(1, heads, 1, 1), 3)
    assert ((a @ v).reshape(N, heads * d, *hw) - ref).abs().max().item() <= 1e-12  # the reference module's order of operations gives the same f64 values
    got = planes_to_nchw(Planes(out.hi.cpu(), out.lo.cpu()), heads * d).double()
    assert ((got - ref).abs() <= bar).all() and _guards_intact(store, 3)


# ------------------------------------------------------------------------------------------------------------------ shortcut
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('scale,hw,pad', [(1, (5, 7), (3, 1)), (2, (3, 5), (1, 3)), (3, (9, 4), (7, 0)), (4, (1, 1), (0, 0)), (2, (17, 33), (15, 15))])
def test_shortcut_is_bit_exact(device, dtype, scale, hw, pad):
    gen = torch.Generator().manual_seed(scale * 100 + hw[0])
    Cc, (h, w) = 3, hw
    x = torch.randn(N, Cc, h, w, generator=gen).to(dtype)
    gamma = (1.0 + 0.5 * torch.randn(1, Cc, 1, 1, generator=gen)).to(dtype)
    oH, oW = (h + pad[0]) * scale, (w + pad[1]) * scale
    out0 = torch.randn(N, Cc, oH, oW, generator=gen).to(dtype)
    want = out0.clone()
    want[:, :, : h * scale, : w * scale] = out0[:, :, : h * scale, : w * scale] + gamma * F.interpolate(x.float(), scale_factor=scale).to(dtype)
    xd, gd, od = x.to(device), gamma.float().reshape(-1).to(device), out0.to(device)
    p = LG3.ShortcutParams()
    p.batch, p.C, p.h, p.w, p.scale, p.out_H, p.out_W, p.dtype = N, Cc, h, w, scale, oH, oW, ops.rsa_dtype(dtype)
    p.x, p.gamma, p.out = xd.data_ptr(), gd.data_ptr(), od.data_ptr()
    assert L.load().rsa_gaterv3_shortcut(C.byref(p), _stream(device)) == 0
    torch.cuda.synchronize()
    assert torch.equal(od.cpu(), want)  # the padded part of out is untouched, the rest equals torch's two roundings


# ------------------------------------------------------------------------------------------------------------------ error codes
def test_error_codes_leave_the_outputs_alone(device):
    lib = L.load()
    dim, hw = 16, (4, 6)
    gen = torch.Generator().manual_seed(3)
    x, w, b, sca_w, sca_b, gamma0, short = _local_inputs(dim, hw, gen)
    xp, _ = _to_planes(x, PF_BF16, True, device)
    out, store = _guarded_planes(N, dim // 8, *hw, PF_BF16, True, device)
    out.hi.fill_(SENTINEL)
    out.lo.fill_(SENTINEL)
    nbytes = lib.rsa_gaterv3_local_workspace_bytes(N, *hw, dim)
    ws = torch.full((nbytes // 4,), SENTINEL, device=device)
    keep = [t.to(device).contiguous() for t in (w.reshape(2 * dim, 18), b, sca_w, sca_b, gamma0, nchw_to_f32map(short))]
    omap = torch.full((N, dim // 4, *hw, 4), SENTINEL, device=device)

    def local(**kw):
        p = LG3.LocalGateParams()
        p.batch, p.H, p.W, p.dim, p.fmt = N, hw[0], hw[1], dim, PF_BF16
        xp.bind(p, 'x')
        out.bind(p, 'out')
        p.weight, p.bias, p.workspace, p.workspace_bytes = keep[0].data_ptr(), keep[1].data_ptr(), ws.data_ptr(), nbytes
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.rsa_gaterv3_local_gate(C.byref(p), _stream(device))

    def sca(**kw):
        p = LG3.ScaApplyParams()
        p.batch, p.H, p.W, p.dim, p.fmt = N, hw[0], hw[1], dim, PF_BF16
        out.bind(p, 's')
        p.sca_w, p.sca_b, p.gamma0, p.short_f32, p.out_f32 = keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), omap.data_ptr()
        p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.rsa_gaterv3_sca_apply(C.byref(p), _stream(device))

    for fn in (local, sca):
        assert fn(batch=0) == E_ARG and fn(fmt=2) == E_ARG and fn(reserved0=1) == E_ARG and fn(workspace=None) == E_ARG
        assert fn(workspace_bytes=nbytes - 16) == E_ARG and fn(dim=12) == E_UNSUPPORTED and fn(dim=520) == E_UNSUPPORTED
        assert fn(workspace=ws.data_ptr() + 4) == E_ALIGN
    assert local(out_hi=xp.hi_ptr()) == E_ARG and local(x_plane_stride=hw[0] * hw[1] - 1) == E_ARG and local(weight=None) == E_ARG
    assert local(out_hi=out.hi_ptr() + 8) == E_ALIGN and sca(s_hi=out.hi_ptr() + 8) == E_ALIGN and sca(gamma0=None) == E_ARG

    Cc, d = 32, 2
    qkv = torch.randn(N, 3 * Cc, *hw, generator=gen)
    qp, _ = _to_planes(qkv, PF_F16, False, device)
    aout, astore = _guarded_planes(N, Cc // 8, *hw, PF_F16, False, device)
    aout.hi.fill_(SENTINEL)
    abytes = lib.rsa_gaterv3_attn_workspace_bytes(N, *hw, 16, d)
    aws = torch.full((abytes // 4,), SENTINEL, device=device)
    temp = torch.ones(16, device=device)

    def attn(**kw):
        p = LG3.AttnParams()
        p.batch, p.H, p.W, p.C, p.heads, p.head_dim, p.fmt = N, hw[0], hw[1], Cc, 16, d, PF_F16
        qp.bind(p, 'qkv')
        aout.bind(p, 'out')
        p.temperature, p.workspace, p.workspace_bytes = temp.data_ptr(), aws.data_ptr(), abytes
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.rsa_gaterv3_channel_attention(C.byref(p), _stream(device))

    assert attn(batch=0) == E_ARG and attn(fmt=3) == E_ARG and attn(reserved0=2) == E_ARG and attn(head_dim=4) == E_ARG and attn(temperature=None) == E_ARG
    assert attn(C=36) == E_UNSUPPORTED and attn(heads=17) == E_UNSUPPORTED and attn(head_dim=65, C=1040) == E_UNSUPPORTED
    assert attn(workspace_bytes=abytes - 16) == E_ARG and attn(out_hi=qp.hi_ptr()) == E_ARG and attn(qkv_plane_stride=1) == E_ARG
    assert attn(qkv_hi=qp.hi_ptr() + 2) == E_ALIGN and attn(workspace=aws.data_ptr() + 8) == E_ALIGN

    y = torch.full((N, 3, 8, 12), SENTINEL, device=device)
    xin = torch.ones(N, 3, 4, 6, device=device)
    gam = torch.ones(3, device=device)

    def shortcut(**kw):
        p = LG3.ShortcutParams()
        p.batch, p.C, p.h, p.w, p.scale, p.out_H, p.out_W, p.dtype = N, 3, 4, 6, 2, 8, 12, L.F32
        p.x, p.gamma, p.out = xin.data_ptr(), gam.data_ptr(), y.data_ptr()
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.rsa_gaterv3_shortcut(C.byref(p), _stream(device))

    assert shortcut(scale=0) == E_ARG and shortcut(scale=9) == E_ARG and shortcut(out_H=7) == E_ARG and shortcut(out_W=11) == E_ARG and shortcut(x=None) == E_ARG
    assert shortcut(dtype=L.U8) == E_UNSUPPORTED and shortcut(dtype=7) == E_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (out.hi, out.lo, ws, omap, aout.hi, aws, y):
        assert bool((t == SENTINEL).all())  # a refused call launches nothing
    assert _guards_intact(store, dim // 8) and _guards_intact(astore, Cc // 8)
