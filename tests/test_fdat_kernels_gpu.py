"""The HIP kernels of csrc/fdat.hip (and rsa_deconv's GELU epilogue) against torch on random data."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from resselt_amd.engine import cugan as CG
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, f32map_to_nchw, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _planes(x, fmt, device):
    p = nchw_to_planes(x.to(device), with_lo=True, fmt=fmt)
    return p, planes_to_nchw(p, x.shape[1])  # the planes and the exact values they hold


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('C_', [48, 108, 180])
@pytest.mark.parametrize('inplace', [True, False])
def test_fdat_interact(device, fmt, mode, C_, inplace):
    g = torch.Generator().manual_seed(C_ + 7 * mode)
    n, H, W = 2, 13, 11
    a, ap = _planes(torch.randn(n, C_, H, W, generator=g), fmt, device)
    c, cp_ = _planes(torch.randn(n, C_, H, W, generator=g), fmt, device)
    x = torch.randn(n, C_, H, W, generator=g).to(device)
    xm = nchw_to_f32map(x)
    xo = xm if inplace else torch.empty_like(xm)
    planes = (C_ + 7) // 8
    cm = torch.rand(n, planes * 8, generator=g).to(device)
    w = (torch.randn(C_, generator=g) / C_**0.5).to(device)
    gamma, beta = (1 + 0.1 * torch.randn(C_, generator=g)).to(device), (0.1 * torch.randn(C_, generator=g)).to(device)
    out = nchw_to_planes(torch.zeros(n, C_, H, W, device=device), with_lo=True, fmt=fmt)
    p = L.FdatInteractParams()
    p.batch, p.H, p.W, p.C, p.mode, p.fmt = n, H, W, C_, mode, fmt
    p.a_hi, p.a_lo, p.a_plane_stride, p.a_batch_stride = a.hi_ptr(), a.lo_ptr(), a.plane_stride, a.batch_stride
    p.c_hi, p.c_lo, p.c_plane_stride, p.c_batch_stride = c.hi_ptr(), c.lo_ptr(), c.plane_stride, c.batch_stride
    p.cm, p.w = cm.data_ptr(), w.data_ptr()
    p.x, p.x_out, p.gamma, p.beta, p.eps = xm.data_ptr(), xo.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.launch('rsa_fdat_interact', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    if mode == 0:
        f = ap * cm[:, :C_, None, None] + cp_
    else:
        f = ap + cp_ * torch.sigmoid((ap * w[None, :, None, None]).sum(1, keepdim=True))
    v = x + f
    ref = F.layer_norm(v.permute(0, 2, 3, 1), (C_,), gamma, beta, 1e-5).permute(0, 3, 1, 2)
    assert (f32map_to_nchw(xo, C_) - v).abs().max().item() <= 1e-5
    tol = 2e-5 if fmt == PF_BF16 else 5e-6  # hi + lo of the normalised output: 16 or 22 significant bits
    assert (planes_to_nchw(out, C_) - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
    if C_ % 8:
        assert out.hi[:, -1, ..., C_ % 8 :].abs().max().item() == 0  # tail channels are zero


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16])
def test_pa_gate(device, fmt):
    g = torch.Generator().manual_seed(5)
    x, xv = _planes(torch.randn(2, 32, 9, 7, generator=g), fmt, device)
    lg, lv = _planes(torch.randn(2, 32, 9, 7, generator=g), fmt, device)
    out = nchw_to_planes(torch.zeros(2, 32, 9, 7, device=device), with_lo=True, fmt=fmt)
    rc = L.load().rsa_pa_gate(x.hi_ptr(), x.lo_ptr(), lg.hi_ptr(), lg.lo_ptr(), x.plane_stride, x.batch_stride, 2, 9, 7, 4, 0.2, fmt, out.hi_ptr(),
                              out.lo_ptr(), _stream(device))  # fmt: skip
    assert rc == 0
    torch.cuda.synchronize()
    ref = F.leaky_relu(xv * torch.sigmoid(lv), 0.2)
    assert (planes_to_nchw(out, 32) - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())  # hi + lo: 16 bits and more


def _lda_q_hr(q, Ho, Wo):
    return F.interpolate(q, (Ho, Wo), mode='bilinear', align_corners=True)


@pytest.mark.parametrize('s,H,W', [(2, 7, 5), (3, 6, 9), (4, 5, 4)])
def test_lda_offsets(device, s, H, W):
    g = torch.Generator().manual_seed(s)
    n, hid = 2, 16
    gc = hid // 2
    q, qv = _planes(torch.randn(n, hid, H, W, generator=g), PF_BF16, device)
    dw = (torch.randn(gc, 9, generator=g) / 3).to(device)
    gamma, beta = (1 + 0.1 * torch.randn(gc, generator=g)).to(device), (0.1 * torch.randn(gc, generator=g)).to(device)
    Ho, Wo = H * s, W * s
    out = nchw_to_planes(torch.zeros(n, hid, Ho, Wo, device=device), with_lo=True)
    p = L.LdaOffsetsParams()
    p.batch, p.H, p.W, p.Hout, p.Wout, p.hidden, p.groups, p.fmt = n, H, W, Ho, Wo, hid, 2, PF_BF16
    p.q_hi, p.q_lo, p.q_plane_stride, p.q_batch_stride = q.hi_ptr(), q.lo_ptr(), q.plane_stride, q.batch_stride
    p.dw_weight, p.gamma, p.beta, p.eps = dw.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-6
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.launch('rsa_lda_offsets', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    t = F.conv2d(_lda_q_hr(qv, Ho, Wo).view(n * 2, gc, Ho, Wo), dw.view(gc, 1, 3, 3), padding=1, groups=gc)
    u = t.mean(1, keepdim=True)
    t = (t - u) / torch.sqrt((t - u).pow(2).mean(1, keepdim=True) + 1e-6) * gamma[:, None, None] + beta[:, None, None]
    ref = F.silu(t).view(n, hid, Ho, Wo)
    assert (planes_to_nchw(out, hid) - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


def _lda_attention_ref(q, k, v, off, rpb, Ho, Wo, scale):
    """LDA_AQU.forward (reference :261-279) from q, k, v and the raw offset-conv output, groups 2, one head."""
    n, hid, H, W = q.shape
    Cv = v.shape[1]
    G = 2
    base = torch.arange(-1, 2, dtype=torch.float32, device=q.device)
    base_off = torch.stack([base.repeat_interleave(3), base.repeat(3)], 1).flatten().view(1, -1, 1, 1)
    o = off.view(n * G, 18, Ho, Wo).tanh() * 11 + base_off
    o = o.view(n * G, 3, 3, 2, Ho, Wo).permute(0, 1, 4, 2, 5, 3)  # b kh h kw w d
    rows, cols = torch.meshgrid(torch.arange(Ho, device=q.device), torch.arange(Wo, device=q.device), indexing='ij')
    idx = torch.stack((rows, cols), -1).view(1, 1, Ho, 1, Wo, 2).float()
    o = (o + idx).contiguous().view(n * G, 3 * Ho, 3 * Wo, 2).clone()
    o[..., 0] = 2 * o[..., 0] / (Ho - 1) - 1
    o[..., 1] = 2 * o[..., 1] / (Wo - 1) - 1
    grid = o.flip(-1)

    def feats(t):
        out = F.grid_sample(t, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        return out.view(n, G, -1, 3, Ho, 3, Wo).permute(0, 4, 6, 3, 5, 1, 2).reshape(n, Ho * Wo, 9, -1)  # b (h w) (kh kw) (g c)

    ks = feats(k.reshape(n * G, hid // G, H, W)) + rpb.view(1, 1, 9, hid)
    vs = feats(v.reshape(n * G, Cv // G, H, W))
    qh = _lda_q_hr(q, Ho, Wo).permute(0, 2, 3, 1).reshape(n, Ho * Wo, 1, hid) * scale
    attn = (qh @ ks.transpose(-1, -2)).softmax(-1)
    return (attn @ vs).view(n, Ho, Wo, Cv).permute(0, 3, 1, 2)


@pytest.mark.parametrize('s,H,W', [(2, 7, 5), (3, 6, 9), (4, 5, 4)])
def test_lda_attention(device, s, H, W):
    g = torch.Generator().manual_seed(10 + s)
    n, hid, Cv = 2, 16, 64
    Ho, Wo = H * s, W * s
    q, qv = _planes(torch.randn(n, hid, H, W, generator=g), PF_BF16, device)
    k, kv = _planes(torch.randn(n, hid, H, W, generator=g), PF_BF16, device)
    v, vv = _planes(torch.randn(n, Cv, H, W, generator=g), PF_BF16, device)
    off = (torch.randn(n, 36, Ho, Wo, generator=g) * 0.8).to(device)  # tanh(o) * 11: many points fall outside the map
    rpb = (0.1 * torch.randn(9, hid, generator=g)).to(device)
    om = nchw_to_f32map(off)
    out = nchw_to_planes(torch.zeros(n, Cv, Ho, Wo, device=device), with_lo=True)
    p = L.LdaAttnParams()
    p.batch, p.H, p.W, p.Hout, p.Wout, p.hidden, p.C, p.groups, p.fmt = n, H, W, Ho, Wo, hid, Cv, 2, PF_BF16
    p.range, p.scale = 11.0, hid**-0.5
    p.q_hi, p.q_lo, p.q_plane_stride, p.q_batch_stride = q.hi_ptr(), q.lo_ptr(), q.plane_stride, q.batch_stride
    p.k_hi, p.k_lo, p.k_plane_stride, p.k_batch_stride = k.hi_ptr(), k.lo_ptr(), k.plane_stride, k.batch_stride
    p.v_hi, p.v_lo, p.v_plane_stride, p.v_batch_stride = v.hi_ptr(), v.lo_ptr(), v.plane_stride, v.batch_stride
    p.offset, p.rpb = om.data_ptr(), rpb.data_ptr()
    p.out_hi, p.out_lo, p.out_plane_stride, p.out_batch_stride = out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride
    L.launch('rsa_lda_attention', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    ref = _lda_attention_ref(qv, kv, vv, off, rpb, Ho, Wo, hid**-0.5)
    err = (planes_to_nchw(out, Cv) - ref).abs().max().item()
    assert err <= 5e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize('cout', [48, 120])
def test_deconv_gelu(device, cout):
    g = torch.Generator().manual_seed(cout)
    n, cin, H, W = 2, 40, 7, 6
    x, xv = _planes(torch.randn(n, cin, H, W, generator=g), PF_BF16, device)
    w = (torch.randn(cin, cout, 4, 4, generator=g) / 20).to(device)
    b = (0.1 * torch.randn(cout, generator=g)).to(device)
    wts = CG.ResampleWeights.make(w, b, 2, 1, True, 3, PF_BF16, device)
    out = nchw_to_planes(torch.zeros(n, cout, 2 * H, 2 * W, device=device), with_lo=True)
    p = CG.resample_params(wts, x, CG.Win(0, 0, H, W), out=out)
    p.act = L.ACT_GELU
    L.launch('rsa_deconv', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    ref = F.gelu(F.conv_transpose2d(xv, w, b, stride=2, padding=1))
    assert (planes_to_nchw(out, cout) - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize('mode', [0, 1])
def test_fdat_interact_alone(device, mode):
    """x NULL: x_out receives the interaction f alone (the first pass of the unfused path)."""
    g = torch.Generator().manual_seed(40 + mode)
    n, C_, H, W = 2, 108, 9, 14
    a, ap = _planes(torch.randn(n, C_, H, W, generator=g), PF_BF16, device)
    c, cp_ = _planes(torch.randn(n, C_, H, W, generator=g), PF_BF16, device)
    cm = torch.rand(n, 8 * ((C_ + 7) // 8), generator=g).to(device)
    w = (torch.randn(C_, generator=g) / C_**0.5).to(device)
    fo = nchw_to_f32map(torch.full((n, C_, H, W), 7.0, device=device))
    p = L.FdatInteractParams()
    p.batch, p.H, p.W, p.C, p.mode, p.fmt = n, H, W, C_, mode, PF_BF16
    p.a_hi, p.a_lo, p.a_plane_stride, p.a_batch_stride = a.hi_ptr(), a.lo_ptr(), a.plane_stride, a.batch_stride
    p.c_hi, p.c_lo, p.c_plane_stride, p.c_batch_stride = c.hi_ptr(), c.lo_ptr(), c.plane_stride, c.batch_stride
    p.cm, p.w, p.x_out = cm.data_ptr(), w.data_ptr(), fo.data_ptr()
    L.launch('rsa_fdat_interact', p, ops.current_stream_ptr(device))
    torch.cuda.synchronize()
    if mode == 0:
        f = ap * cm[:, :C_, None, None] + cp_
    else:
        f = ap + cp_ * torch.sigmoid((ap * w[None, :, None, None]).sum(1, keepdim=True))
    assert (f32map_to_nchw(fo, C_) - f).abs().max().item() <= 1e-5
