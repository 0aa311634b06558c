"""GPU checks of the OmniSR kernels (csrc/omnisr.hip) against plain torch on ragged shapes: both token mappings of both attentions with
Hp != Wp and head widths 8, 12 and 16, the gated FFN middle, the SiLU mode of rsa_channel_gate with rsa_omni_gate_scale, and the ESA
convolution / max-pool / apply kernels."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import Planes, f32map_to_nchw, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu
HEADS = 4


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _qkv(n, d, H, W, seed):
    """q, k, v [n, heads, d, H, W] and their head-padded planes."""
    g = torch.Generator().manual_seed(seed)
    hp = (d + 7) // 8
    qkv = torch.randn((3, n, HEADS, d, H, W), generator=g)
    padded = torch.zeros((n, 3, HEADS, hp * 8, H, W))
    padded[:, :, :, :d] = qkv.permute(1, 0, 2, 3, 4, 5)
    return qkv, padded.reshape(n, 3 * HEADS * hp * 8, H, W), hp


def _tokens(t, ws, grid, window_attn):
    """[n, h, d, H, W] -> [n, sets, h, tokens, d] in the reference's token order."""
    n, h, d, H, W = t.shape
    if window_attn and grid:  # 'b d (w1 x) (w2 y) -> b x y w1 w2 d'
        t = t.reshape(n, h, d, ws, H // ws, ws, W // ws).permute(0, 4, 6, 1, 3, 5, 2)
    elif window_attn or not grid:  # 'b d (x w1) (y w2)'
        t = t.reshape(n, h, d, H // ws, ws, W // ws, ws).permute(0, 3, 5, 1, 4, 6, 2)
    else:  # channel attention grid: '(h ph) (w pw) -> (ph pw) ... (h w)'
        t = t.reshape(n, h, d, H // ws, ws, W // ws, ws).permute(0, 4, 6, 1, 3, 5, 2)
    return t.reshape(n, t.shape[1] * t.shape[2], h, -1, d)


def _untokens(o, ws, grid, window_attn, H, W):
    n, _, h, _, d = o.shape
    if window_attn and grid:
        o = o.reshape(n, H // ws, W // ws, h, ws, ws, d).permute(0, 3, 6, 4, 1, 5, 2)
    elif window_attn or not grid:
        o = o.reshape(n, H // ws, W // ws, h, ws, ws, d).permute(0, 3, 6, 1, 4, 2, 5)
    else:
        o = o.reshape(n, ws, ws, h, H // ws, W // ws, d).permute(0, 3, 6, 4, 1, 5, 2)
    return o.reshape(n, h, d, H, W)


def _params(qkv_pl, out_pl, n, H, W, ws, d, grid):
    p = L.OmniAttnParams()
    p.batch, p.H, p.W, p.ws, p.heads, p.head_dim, p.grid, p.fmt = n, H, W, ws, HEADS, d, grid, 0
    p.qkv_hi, p.qkv_lo, p.qkv_plane_stride, p.qkv_batch_stride = qkv_pl.hi_ptr(), qkv_pl.lo_ptr(), qkv_pl.plane_stride, qkv_pl.batch_stride
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out_pl.hi_ptr(), out_pl.lo_ptr(), out_pl.plane_stride, out_pl.batch_stride
    return p


def _heads_out(out_pl, n, d, hp, H, W):
    o = planes_to_nchw(out_pl, HEADS * hp * 8).cpu().reshape(n, HEADS, hp * 8, H, W)
    assert torch.all(o[:, :, d:] == 0)
    return o[:, :, :d]


@pytest.mark.parametrize('grid', [0, 1])
@pytest.mark.parametrize('d,ws,pe', [(16, 8, True), (12, 4, True), (8, 8, False), (11, 4, False)])
def test_window_attention(device, grid, d, ws, pe):
    n, H, W = 2, 2 * ws, 3 * ws
    qkv, padded, hp = _qkv(n, d, H, W, 11 + d + grid)
    qkv[0] *= d**-0.5  # q arrives pre-scaled, as the model folds head_dim^-0.5 into to_qkv
    padded[:, : HEADS * hp * 8] *= d**-0.5
    qkv_pl = nchw_to_planes(padded.to(device))
    out_pl = Planes.empty(n, HEADS * hp, H, W, device)
    p = _params(qkv_pl, out_pl, n, H, W, ws, d, grid)
    table = torch.randn(((2 * ws - 1) ** 2, HEADS)) if pe else None
    if pe:
        tb = table.to(device)
        p.bias_table = tb.data_ptr()
    L.launch('rsa_omni_window_attention', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    got = _heads_out(out_pl, n, d, hp, H, W)
    # reference on the pre-scaled q
    q, k, v = (_tokens(t.double(), ws, grid, True) for t in qkv)
    sim = torch.einsum('nshid,nshjd->nshij', q, k)
    if pe:
        pos = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing='ij')).reshape(2, -1)
        rel = pos[:, :, None] - pos[:, None, :] + ws - 1
        idx = rel[0] * (2 * ws - 1) + rel[1]
        sim = sim + table.double()[idx].permute(2, 0, 1)
    o = torch.einsum('nshij,nshjd->nshid', sim.softmax(-1), v)
    want = _untokens(o, ws, grid, True, H, W).float()
    err = (got - want).abs().max().item()
    assert err < 1e-4, err


@pytest.mark.parametrize('grid', [0, 1])
@pytest.mark.parametrize('d,ws,H,W', [(16, 8, 16, 24), (12, 4, 28, 12), (8, 8, 80, 72), (11, 4, 8, 12)])
def test_channel_attention(device, grid, d, ws, H, W):
    n = 2
    qkv, padded, hp = _qkv(n, d, H, W, 21 + d + grid)
    qkv_pl = nchw_to_planes(padded.to(device))
    out_pl = Planes.empty(n, HEADS * hp, H, W, device)
    p = _params(qkv_pl, out_pl, n, H, W, ws, d, grid)
    temp = (torch.rand(HEADS) + 0.5).to(device)
    wsb = int(L.load().rsa_omni_channel_attn_workspace_bytes(n, H, W, ws, HEADS, d, grid))
    work = torch.empty(wsb // 4, dtype=torch.float32, device=device)
    p.temperature, p.workspace = temp.data_ptr(), work.data_ptr()
    L.launch('rsa_omni_channel_attention', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    got = _heads_out(out_pl, n, d, hp, H, W)
    q, k, v = (_tokens(t.double(), ws, grid, False).transpose(-1, -2) for t in qkv)  # [n, sets, h, d, tokens]
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = (q @ k.transpose(-1, -2)) * temp.cpu().double()[None, None, :, None, None]
    o = (attn.softmax(-1) @ v).transpose(-1, -2)
    want = _untokens(o, ws, grid, False, H, W).float()
    err = (got - want).abs().max().item()
    assert err < 1e-4, err


@pytest.mark.parametrize('c,H,W', [(48, 13, 29), (44, 7, 5)])
def test_gelu_gate_dwconv(device, c, H, W):
    n, cp = 2, (c + 7) // 8
    g = torch.Generator().manual_seed(c)
    x = torch.randn((n, 2 * c, H, W), generator=g)
    w = torch.randn((2 * c, 1, 3, 3), generator=g) / 3
    xin = torch.zeros((n, 2 * cp * 8, H, W))
    xin[:, :c], xin[:, cp * 8 : cp * 8 + c] = x[:, :c], x[:, c:]
    wk = torch.zeros((2 * cp * 8, 9))
    wk[:c], wk[cp * 8 : cp * 8 + c] = w[:c].reshape(c, 9), w[c:].reshape(c, 9)
    src = nchw_to_planes(xin.to(device))
    out = Planes.empty(n, cp, H, W, device)
    wd = wk.to(device)
    p = L.GeluGateDwConvParams()
    p.batch, p.H, p.W, p.planes, p.fmt = n, H, W, cp, 0
    p.in_hi, p.in_lo, p.in_plane_stride, p.in_batch_stride = src.hi_ptr(), src.lo_ptr(), src.plane_stride, src.batch_stride
    p.weight = wd.data_ptr()
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.launch('rsa_gelu_gate_dwconv', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    x1, x2 = F.conv2d(x.double(), w.double(), padding=1, groups=2 * c).chunk(2, dim=1)
    want = (F.gelu(x1) * x2).float()
    got = planes_to_nchw(out, c).cpu()
    assert (got - want).abs().max().item() < 1e-4


def test_silu_channel_gate_and_scale(device):
    n, c, H, W, hid = 2, 44, 37, 23, 11
    cp = (c + 7) // 8
    g = torch.Generator().manual_seed(5)
    h = torch.randn((n, c, H, W), generator=g)
    wa, wb = torch.randn((hid, c), generator=g) / 4, torch.randn((c, hid), generator=g) / 2
    pl = nchw_to_planes(h.to(device))
    w1 = torch.zeros((hid, cp * 8))
    w1[:, :c] = wa
    w2 = torch.zeros((cp * 8, hid))
    w2[:c] = wb
    w1, w2, b1, b2 = w1.to(device), w2.to(device), torch.zeros(hid, device=device), torch.zeros(cp * 8, device=device)
    gate = torch.empty((n, cp * 8), device=device)
    work = torch.empty(int(L.load().rsa_channel_gate_workspace_bytes(n, H, W, cp)) // 4, device=device)
    gp = L.ChannelGateParams()
    gp.batch, gp.H, gp.W, gp.planes, gp.hidden, gp.relu, gp.fmt = n, H, W, cp, hid, 3, 0
    gp.in_hi, gp.in_lo, gp.in_plane_stride, gp.in_batch_stride = pl.hi_ptr(), pl.lo_ptr(), pl.plane_stride, pl.batch_stride
    gp.w1, gp.b1, gp.w2, gp.b2, gp.workspace, gp.gate = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), work.data_ptr(), gate.data_ptr()
    L.launch('rsa_channel_gate', gp, ops.current_stream_ptr(device))
    lib = L.load()
    L.check(lib.rsa_omni_gate_scale(pl.hi_ptr(), pl.lo_ptr(), pl.plane_stride, pl.batch_stride, n, H, W, cp, gate.data_ptr(), 0, pl.hi_ptr(), pl.lo_ptr(),
                                    C.c_void_p(ops.current_stream_ptr(device))), 'rsa_omni_gate_scale')  # fmt: skip
    torch.cuda.synchronize()
    gref = torch.sigmoid(F.silu(h.double().mean((2, 3)) @ wa.double().T) @ wb.double().T)
    assert (gate[:, :c].cpu() - gref.float()).abs().max().item() < 1e-5
    assert (planes_to_nchw(pl, c).cpu() - (h.double() * gref[:, :, None, None]).float()).abs().max().item() < 1e-4


@pytest.mark.parametrize('stride,pad,H,W', [(2, 0, 24, 17), (1, 1, 5, 3), (2, 0, 15, 16)])
def test_esa_conv3x3(device, stride, pad, H, W):
    n, f = 2, 16
    g = torch.Generator().manual_seed(H)
    x, w, b = torch.randn((n, f, H, W), generator=g), torch.randn((f, f, 3, 3), generator=g) / 12, torch.randn(f, generator=g)
    want = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad).float()
    Ho, Wo = want.shape[2:]
    src, out = nchw_to_f32map(x.to(device)), torch.empty((n, f // 4, Ho, Wo, 4), device=device)
    wd, bd = w.to(device), b.to(device)
    p = L.EsaConvParams()
    p.batch, p.H, p.W, p.Hout, p.Wout, p.cin, p.cout, p.stride, p.pad = n, H, W, Ho, Wo, f, f, stride, pad
    p.in_, p.weight, p.bias, p.out = src.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    L.launch('rsa_esa_conv3x3', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    assert (f32map_to_nchw(out, f).cpu() - want).abs().max().item() < 1e-4


@pytest.mark.parametrize('H,W', [(7, 7), (20, 11), (31, 64)])
def test_esa_maxpool(device, H, W):
    n, f = 2, 20
    x = torch.randn((n, f, H, W))
    want = F.max_pool2d(x, kernel_size=7, stride=3)
    src = nchw_to_f32map(x.to(device))
    out = torch.empty((n, 5, want.shape[2], want.shape[3], 4), device=device)
    L.check(L.load().rsa_esa_maxpool(src.data_ptr(), n, f, H, W, out.data_ptr(), C.c_void_p(ops.current_stream_ptr(device))), 'rsa_esa_maxpool')
    torch.cuda.synchronize()
    assert torch.equal(f32map_to_nchw(out, f).cpu(), want)


@pytest.mark.parametrize('c,f,H,W,Hc,Wc', [(64, 16, 24, 40, 2, 5), (44, 16, 17, 9, 1, 1), (128, 32, 16, 16, 3, 2)])
def test_esa_apply(device, c, f, H, W, Hc, Wc):
    n = 2
    g = torch.Generator().manual_seed(c + H)
    x, c1, c3 = torch.randn((n, c, H, W), generator=g), torch.randn((n, f, H, W), generator=g), torch.randn((n, f, Hc, Wc), generator=g)
    wf, bf = torch.randn((f, f), generator=g) / 4, torch.randn(f, generator=g)
    w4, b4 = torch.randn((c, f), generator=g) / 4, torch.randn(c, generator=g)
    up = F.interpolate(c3.double(), (H, W), mode='bilinear', align_corners=False)
    cf = torch.einsum('oi,nihw->nohw', wf.double(), c1.double()) + bf.double()[:, None, None]
    m = torch.sigmoid(torch.einsum('oi,nihw->nohw', w4.double(), up + cf) + b4.double()[:, None, None])
    want = (x.double() * m).float()
    xm, c1m, c3m = (nchw_to_f32map(t.to(device)) for t in (x, c1, c3))
    dev = [t.to(device) for t in (wf, bf, w4, b4)]
    pl = Planes.empty(n, (c + 7) // 8, H, W, device)
    p = L.EsaApplyParams()
    p.batch, p.H, p.W, p.C, p.f, p.Hc, p.Wc, p.fmt = n, H, W, c, f, Hc, Wc, 0
    p.x, p.c1, p.c3, p.out = xm.data_ptr(), c1m.data_ptr(), c3m.data_ptr(), xm.data_ptr()  # in place
    p.wf, p.bf, p.w4, p.b4 = (t.data_ptr() for t in dev)
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = pl.hi_ptr(), pl.lo_ptr(), pl.plane_stride, pl.batch_stride
    L.launch('rsa_esa_apply', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    assert (f32map_to_nchw(xm, c).cpu() - want).abs().max().item() < 1e-4
    assert (planes_to_nchw(pl, c).cpu() - want).abs().max().item() < 1e-4
