"""GPU checks of the ATD kernels (csrc/atd.hip) against plain torch, each on its own inputs.

- rsa_atd_dict + rsa_atd_ca: sim against torch f32 (the largest relative error is printed: it is the figure DESIGN.md records; the near-tie
  threshold TAU = 1e-4 must be at least 10 times it), ids EXACTLY the first maximum of the kernel's own sim (rows with repeated maxima
  included), sim V against torch.
- rsa_atd_sort: EXACTLY torch.sort(stable=True), and its inverse.
- rsa_atd_attention in both modes: ragged last group, flipped-tail padding, shift, head widths 12 / 32 / 35 / 64, groups of 64 / 128 / 256,
  permutation supplied by the test.
- rsa_atd_dwconv, and rsa_atd_refine on an n that is not a power of two with one dictionary token never chosen.
"""

import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import Planes, nchw_to_f32map, f32map_to_nchw, nchw_to_planes, planes_to_nchw
from resselt_amd.engine.transformer import relative_position_index

pytestmark = pytest.mark.gpu
TAU = 1e-4


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return ops.current_stream_ptr(device)


def _ca(device, b, H, W, Cc, m, rc, products, xn, wq, bq, wk, bk, wv, bv, scale, td):
    n = H * W
    Cp = (Cc + 31) // 32 * 32
    kn = torch.empty(b, m, 16, device=device)
    vt_hi = torch.empty(b, Cp, 128, dtype=torch.bfloat16, device=device)
    vt_lo = torch.empty_like(vt_hi)
    dp = L.AtdDictParams()
    dp.batch, dp.C, dp.m, dp.rc = b, Cc, m, rc
    dp.td, dp.wk, dp.bk, dp.wv, dp.bv = td.data_ptr(), wk.data_ptr(), bk.data_ptr(), wv.data_ptr(), bv.data_ptr()
    dp.kn, dp.vt_hi, dp.vt_lo = kn.data_ptr(), vt_hi.data_ptr(), vt_lo.data_ptr()
    L.launch('rsa_atd_dict', dp, _stream(device))
    xmap = nchw_to_f32map(xn.transpose(1, 2).reshape(b, Cc, H, W))
    sim = torch.empty(b, n, m, device=device)
    ids = torch.empty(b, n, dtype=torch.int32, device=device)
    out = torch.empty_like(xmap)
    ap = L.AtdCaParams()
    ap.batch, ap.H, ap.W, ap.C, ap.m, ap.rc, ap.products = b, H, W, Cc, m, rc, products
    ap.xn, ap.wq, ap.bq, ap.kn, ap.scale = xmap.data_ptr(), wq.data_ptr(), bq.data_ptr(), kn.data_ptr(), scale.data_ptr()
    ap.vt_hi, ap.vt_lo, ap.sim, ap.ids, ap.out = vt_hi.data_ptr(), vt_lo.data_ptr(), sim.data_ptr(), ids.data_ptr(), out.data_ptr()
    L.launch('rsa_atd_ca', ap, _stream(device))
    torch.cuda.synchronize()
    return sim, ids, f32map_to_nchw(out, Cc).flatten(2).transpose(1, 2)


@pytest.mark.parametrize('Cc,m,rc,H,W,b', [(48, 64, 8, 13, 19, 2), (210, 128, 10, 24, 21, 1), (64, 50, 4, 9, 15, 1), (256, 128, 16, 16, 16, 1)])
@pytest.mark.parametrize('products', [3, 1])
def test_dictionary_cross_attention(device, Cc, m, rc, H, W, b, products):
    g = torch.Generator().manual_seed(Cc + m)
    r = lambda *s: torch.randn(*s, generator=g).to(device)  # noqa: E731
    n = H * W
    xn, td = r(b, n, Cc), r(b, m, Cc)
    wq, bq, wk, bk = r(rc, Cc) / math.sqrt(Cc), r(rc) * 0.1, r(rc, Cc) / math.sqrt(Cc), r(rc) * 0.1
    wv, bv = r(Cc, Cc) / math.sqrt(Cc), r(Cc) * 0.1
    scale = 1 + torch.rand(m, generator=g).to(device) * math.log(m)
    sim, ids, out = _ca(device, b, H, W, Cc, m, rc, products, xn, wq, bq, wk, bk, wv, bv, scale, td)
    q, k, v = F.linear(xn, wq, bq), F.linear(td, wk, bk), F.linear(td, wv, bv)
    ref = ((F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * scale).softmax(-1)
    rel = ((sim - ref).abs() / ref.abs().clamp_min(1e-30))[ref > 1e-6].max().item()
    top = ((sim - ref).abs().max(-1).values / ref.max(-1).values).max().item()
    print(f'C {Cc} m {m} rc {rc}: sim max relative error {rel:.3e}, relative to the row maximum {top:.3e}')
    assert top * 10 <= TAU
    assert torch.equal(ids.long(), sim.argmax(-1))
    want = ref @ v
    err = (out - want).abs().max().item()
    assert err <= (3e-5 if products == 3 else 2e-2) * max(1.0, want.abs().max().item()), err


def test_ids_are_the_first_maximum_on_ties(device):
    """Identical dictionary rows give bit-identical logits: the id must be the lowest index among them."""
    g = torch.Generator().manual_seed(9)
    Cc, m, rc, H, W = 48, 64, 8, 16, 12
    xn = torch.randn(1, H * W, Cc, generator=g).to(device)
    td = torch.randn(1, m, Cc, generator=g)
    td[0, 40] = td[0, 3]
    td[0, 9] = td[0, 3]
    td[0, 63] = td[0, 17]
    td = td.to(device)
    r = lambda *s: torch.randn(*s, generator=g).to(device)  # noqa: E731
    wq, wk, wv = r(rc, Cc) / 7, r(rc, Cc) / 7, r(Cc, Cc) / 7
    z = torch.zeros(Cc, device=device)
    scale = torch.full((m,), 3.0, device=device)
    sim, ids, _ = _ca(device, 1, H, W, Cc, m, rc, 3, xn, wq, z[:rc], wk, z[:rc], wv, z, scale, td)
    assert torch.equal(sim[..., 3], sim[..., 9]) and torch.equal(sim[..., 3], sim[..., 40]) and torch.equal(sim[..., 17], sim[..., 63])
    assert torch.equal(ids.long(), sim.argmax(-1))
    assert not (ids == 40).any() and not (ids == 9).any() and not (ids == 63).any()
    assert (ids == 3).any() or (ids == 17).any()


@pytest.mark.parametrize('b,n,m', [(1, 200, 64), (2, 2048, 128), (1, 5000, 7), (3, 70001, 128), (1, 256, 1)])
def test_sort_is_the_stable_sort(device, b, n, m):
    g = torch.Generator().manual_seed(n)
    ids = torch.randint(0, m, (b, n), generator=g, dtype=torch.int32)
    ids[:, : n // 3] = ids[:, : n // 3] % max(1, m // 8)  # skewed: long runs of one category
    ids = ids.to(device)
    lib = L.load()
    perm = torch.full((b, n), -1, dtype=torch.int32, device=device)
    inv = torch.full((b, n), -1, dtype=torch.int32, device=device)
    ws = torch.empty(int(lib.rsa_atd_sort_workspace_bytes(b, n)), dtype=torch.uint8, device=device)
    L.check(lib.rsa_atd_sort(ids.data_ptr(), b, n, m, perm.data_ptr(), inv.data_ptr(), ws.data_ptr(), C.c_void_p(_stream(device))), 'rsa_atd_sort')
    torch.cuda.synchronize()
    want = torch.sort(ids.long(), dim=-1, stable=True).indices
    assert torch.equal(perm.long(), want)
    assert torch.equal(torch.gather(inv.long(), 1, want), torch.arange(n, device=device).expand(b, n))


def _attention(device, qkv, heads, hd, mode, ws, shift, gs, products, scale, table, perm, H, W):
    """qkv [b, n, 3, heads, hd] f32 -> the kernel's output [b, n, heads, hd]."""
    b, n = qkv.shape[:2]
    hp = (hd + 7) // 8
    padded = torch.zeros(b, n, 3, heads, hp * 8, device=device)
    padded[..., :hd] = qkv
    pl = nchw_to_planes(padded.reshape(b, n, -1).transpose(1, 2).reshape(b, -1, H, W), with_lo=True)
    out = Planes.empty(b, heads * hp, H, W, device, True)
    out.hi.fill_(7.0)
    out.lo.zero_()
    p = L.AtdAttnParams()
    p.batch, p.H, p.W, p.heads, p.head_dim, p.mode, p.ws, p.shift, p.gs, p.products, p.scale = b, H, W, heads, hd, mode, ws, shift, gs, products, scale
    p.qkv_hi, p.qkv_lo, p.qkv_plane_stride, p.qkv_batch_stride = pl.hi_ptr(), pl.lo_ptr(), pl.plane_stride, pl.batch_stride
    p.bias_table = None if table is None else table.data_ptr()
    p.perm = None if perm is None else perm.data_ptr()
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.launch('rsa_atd_attention', p, _stream(device))
    torch.cuda.synchronize()
    y = planes_to_nchw(out, heads * hp * 8).flatten(2).transpose(1, 2).reshape(b, n, heads, hp * 8)
    assert y[..., hd:].abs().max().item() == 0 if hp * 8 > hd else True
    return y[..., :hd]


@pytest.mark.parametrize('hd,heads,gs,n_hw', [(12, 4, 128, (24, 24)), (35, 6, 256, (20, 27)), (32, 2, 256, (8, 16)), (64, 2, 64, (13, 15)), (35, 2, 256, (32, 32)),
                                             (12, 3, 200, (10, 20))])  # fmt: skip
@pytest.mark.parametrize('products', [3, 1])
def test_category_attention(device, hd, heads, gs, n_hw, products):
    H, W = n_hw
    n, b = H * W, 2
    g = torch.Generator().manual_seed(hd * 100 + gs)
    qkv = torch.randn(b, n, 3, heads, hd, generator=g).to(device)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).to(device)
    gsz = min(n, gs)
    scale = 1.7 / math.sqrt(hd)
    y = _attention(device, qkv, heads, hd, 1, 8, 0, gsz, products, scale, None, perm.to(torch.int32).contiguous(), H, W)
    ng = (n + gsz - 1) // gsz
    sh = torch.gather(qkv.reshape(b, n, -1), 1, perm[..., None].expand(-1, -1, 3 * heads * hd))
    pad_n = ng * gsz - n
    t = torch.cat((sh, torch.flip(sh[:, n - pad_n : n], dims=[1])), 1).reshape(b, ng, gsz, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)
    o = ((t[0] @ t[1].transpose(-2, -1) * scale).softmax(-1) @ t[2]).permute(0, 1, 3, 2, 4).reshape(b, n + pad_n, heads, hd)[:, :n]
    inv = torch.empty_like(perm)
    inv.scatter_(1, perm, torch.arange(n, device=device).expand(b, n))
    want = torch.gather(o.reshape(b, n, -1), 1, inv[..., None].expand(-1, -1, heads * hd)).reshape(b, n, heads, hd)
    err = (y - want).abs().max().item()
    print(f'category hd {hd} gs {gsz} n {n} products {products}: max-abs {err:.3e}')
    assert err <= (5e-5 if products == 3 else 3e-2) * max(1.0, want.abs().max().item()), err


@pytest.mark.parametrize('hd,heads,ws,shift,n_hw', [(12, 4, 8, 0, (16, 24)), (12, 4, 8, 4, (16, 24)), (35, 6, 16, 8, (32, 48)), (64, 1, 16, 0, (16, 32)), (32, 2, 4, 2, (8, 12)),
                                                   (35, 2, 8, 4, (24, 8))])  # fmt: skip
@pytest.mark.parametrize('products', [3, 1])
def test_window_attention(device, hd, heads, ws, shift, n_hw, products):
    H, W = n_hw
    n, b = H * W, 2
    g = torch.Generator().manual_seed(hd + ws + shift)
    qkv = torch.randn(b, n, 3, heads, hd, generator=g).to(device)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).to(device)
    scale = hd**-0.5
    y = _attention(device, qkv, heads, hd, 0, ws, shift, 1, products, scale, table.t().contiguous(), None, H, W)
    c = heads * hd
    t = qkv.reshape(b, H, W, 3 * c)
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    xw = t.view(b, H // ws, ws, W // ws, ws, 3 * c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = (xw[0] * scale) @ xw[1].transpose(-2, -1)
    rpi = relative_position_index(ws).to(device)
    a = a + table[rpi.reshape(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1).unsqueeze(0)
    if shift:
        from resselt_amd.engine.transformer import shift_mask

        mask = shift_mask(H, W, (ws, ws), (shift, shift)).to(device)
        nw = mask.shape[0]
        a = (a.view(b, nw, heads, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, ws * ws, ws * ws)
    o = (a.softmax(-1) @ xw[2]).transpose(1, 2).reshape(-1, ws, ws, c)
    o = o.view(b, H // ws, W // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, H, W, c)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    want = o.reshape(b, n, heads, hd)
    err = (y - want).abs().max().item()
    print(f'window hd {hd} ws {ws} shift {shift} products {products}: max-abs {err:.3e}')
    assert err <= (5e-5 if products == 3 else 3e-2) * max(1.0, want.abs().max().item()), err


@pytest.mark.parametrize('c,H,W', [(96, 13, 17), (420, 9, 30)])
def test_dwconv_gelu_residual(device, c, H, W):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(2, c, H, W, generator=g).to(device)
    w = (torch.randn(c, 1, 5, 5, generator=g) / 5).to(device)
    bias = (torch.randn(c, generator=g) / 5).to(device)
    P = (c + 7) // 8
    src = nchw_to_planes(x, with_lo=True)
    out = Planes.empty(2, P, H, W, device, True)
    wp = torch.zeros(P * 8, 25, device=device)
    bp = torch.zeros(P * 8, device=device)
    wp[:c], bp[:c] = w.reshape(c, 25), bias
    p = L.AtdDwConvParams()
    p.batch, p.H, p.W, p.planes = 2, H, W, P
    p.in_hi, p.in_lo, p.in_plane_stride, p.in_batch_stride = src.hi_ptr(), src.lo_ptr(), src.plane_stride, src.batch_stride
    p.weight, p.bias = wp.data_ptr(), bp.data_ptr()
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.launch('rsa_atd_dwconv', p, _stream(device))
    torch.cuda.synchronize()
    xs = planes_to_nchw(src, c)
    want = xs + F.gelu(F.conv2d(xs, w, bias, padding=2, groups=c))
    assert (planes_to_nchw(out, c) - want).abs().max().item() <= 3e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('Cc,m,H,W,b', [(48, 64, 23, 47, 2), (210, 128, 40, 52, 1), (64, 50, 9, 13, 1)])
def test_refinement(device, Cc, m, H, W, b):
    """n is not a power of two (and not a multiple of the 1024-pixel chunk); dictionary token 5 is never the maximum of any pixel."""
    g = torch.Generator().manual_seed(m + H)
    n = H * W
    logits = torch.randn(b, n, m, generator=g) * 2
    logits[..., 5] = -9.0
    sim = logits.softmax(-1).to(device).contiguous()
    assert not (sim.argmax(-1) == 5).any()
    x = torch.randn(b, n, Cc, generator=g).to(device)
    td = torch.randn(b, m, Cc, generator=g).to(device)
    gamma, beta = (1 + torch.randn(m, generator=g) / 4).to(device), (torch.randn(m, generator=g) / 4).to(device)
    sigma = torch.randn(m, 1, generator=g).to(device)
    z = F.instance_norm(sim.transpose(-1, -2), weight=gamma, bias=beta, eps=1e-5)
    s = torch.sigmoid(sigma)
    want = s * td + (1 - s) * torch.einsum('btn,bnc->btc', z.double().softmax(-1), x.double()).float()
    lib = L.load()
    ws = torch.empty(int(lib.rsa_atd_refine_workspace_bytes(b, H, W, Cc, m)), dtype=torch.uint8, device=device)
    xmap = nchw_to_f32map(x.transpose(1, 2).reshape(b, Cc, H, W))
    tdk = td.clone()
    p = L.AtdRefineParams()
    p.batch, p.H, p.W, p.C, p.m, p.eps = b, H, W, Cc, m, 1e-5
    sg = sigma.reshape(-1).contiguous()
    p.sim, p.x, p.gamma, p.beta, p.sigma, p.td, p.workspace = sim.data_ptr(), xmap.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sg.data_ptr(), tdk.data_ptr(), ws.data_ptr()
    L.launch('rsa_atd_refine', p, _stream(device))
    torch.cuda.synchronize()
    err = (tdk - want).abs().max().item()
    print(f'refine C {Cc} m {m} n {n}: max-abs {err:.3e}')
    assert err <= 2e-5 * max(1.0, want.abs().max().item()), err
    tdk2 = td.clone()
    p.td = tdk2.data_ptr()
    L.launch('rsa_atd_refine', p, _stream(device))
    torch.cuda.synchronize()
    assert torch.equal(tdk, tdk2)  # fixed reduction order: bit-identical
