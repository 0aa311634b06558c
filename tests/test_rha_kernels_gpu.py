"""RHA's kernels through the C-ABI against f64 formulas that are given exactly the values the planes hold.

Bounds (derived, not measured; every case prints a MEASURE line).

Window attention.  The kernel reads the planes' values, computes in f32 and writes an f32 map, so no plane rounding enters and the bound is
the same for bf16 hi + lo and fp16 hi-only inputs.  Roundings behind one output value, each 2^-24 relative to the sum it belongs to: the qkv
product (C2 <= 32 terms + bias + positional term + scaling: 36), the focusing (two norms of 32 terms, the cube, two divisions: 70, of which
the cube counts three times), k^T v over N <= 64 tokens (64), q kv and the normaliser (2 d + 3 <= 11), the 5x5 of v (26), proj (33): about
250 roundings, 250 * 2^-24 = 1.5e-5 if they all add up; the sums they are relative to can exceed the result by cancellation, for which a
factor 2 is allowed: 3e-5 * |out|max.
Mix.  The 5x5 is 25 terms + bias in f32 (26 * 2^-24 = 1.6e-6 relative to sum |w x| <= about 2 |out|max) and the bilinear sample 4 terms with
exact weights (down is a power of two) in 7 roundings; the result is stored as split planes: hi + lo bf16 keeps 16 bits (2^-17 = 7.6e-6
relative), fp16 hi alone rounds by up to 2^-11.  Bound: (2^-17 + 4e-6) * |out|max = 1.2e-5 * |out|max with lo halves, (2^-11 + 4e-6) on fp16
hi planes.
Gate.  expf within 2 ulp, t / (t + 2), three products: under 12 roundings, 7e-7, + the plane store: 1e-5 * |out|max with lo halves.

Shapes: pooled grids of one window and of 2 x 3 windows, window 4 and 8, shift 0 and window / 2 (with Hd = window the shifted window wraps onto
itself), down 1 / 2 / 4 / 8, C2 8 / 24 / 32, batch 2, x2 at a plane offset inside a wider buffer.  Every attention case carries a pool cell
whose values are all negative, a token whose q and k pre-activations are all negative and a channel with scale = 6.  Mix: maps a few
pooled pixels wide that cross the 32 x 8 tile edges.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import rha_oracle as O
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16, Planes, f32map_to_nchw, nchw_to_f32map, nchw_to_planes, planes_to_nchw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _to(pl, device):
    return Planes(pl.hi.to(device), None if pl.lo is None else pl.lo.to(device))


# ------------------------------------------------------------------------------------------------------------------ window attention
def _attn_params(c2, ws, g):
    d, n = c2 // 8, ws * ws
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    sd = {'a.qkv.weight': r(3 * c2, c2) / c2**0.5, 'a.qkv.bias': r(3 * c2) * 0.2, 'a.positional_encoding': r(1, n, c2) * 0.5, 'a.scale': r(1, 1, c2) * 0.7,
          'a.proj.weight': r(c2, c2) / c2**0.5, 'a.proj.bias': r(c2) * 0.2, 'a.dwc.weight': r(d, 1, 5, 5) / 5, 'a.dwc.bias': r(d) * 0.1}  # fmt: skip
    sd['a.scale'][0, 0, 3] = 6.0  # softplus 6.0025: (1e-6 / 6)^3 squared is subnormal
    sd['a.positional_encoding'][0, 5] = -50.0  # token 5 of every window: every k pre-activation negative
    return sd


def _attn_want(held, sd, down, ws, shift):
    x = F.max_pool2d(held, down, down) if down > 1 else held
    x = torch.roll(x, (-shift, -shift), (2, 3))
    y = O.window_attention({k: v.double() for k, v in sd.items()}, 'a', x, ws)
    return torch.roll(y, (shift, shift), (2, 3))


def _attn_run(device, c2, ws, down, shift, n, grid, fmt, with_lo, off, seed):
    g = torch.Generator().manual_seed(seed)
    sd = _attn_params(c2, ws, g)
    Hd, Wd = grid[0] * ws, grid[1] * ws
    H, W = Hd * down, Wd * down
    planes = off + c2 // 8 + 1  # a wider buffer: other planes before and behind x2
    x = torch.randn((n, planes * 8, H, W), generator=g)
    ch = slice(8 * off, 8 * off + c2)
    x[0, ch, down : 2 * down, 0:down] = -x[0, ch, down : 2 * down, 0:down].abs() - 0.1  # a pool cell of negative values only
    u = torch.linalg.solve(sd['a.qkv.weight'][:c2].double(), -torch.ones(c2, dtype=torch.float64)).float()  # Wq u = -1
    x[n - 1, ch, 0:down, 0:down] = (50.0 * u)[:, None, None]  # pooled token (0, 0) of the last image: every q pre-activation is about -50
    pl = nchw_to_planes(x, with_lo, fmt)
    held = planes_to_nchw(pl, planes * 8)[:, ch].double()  # the values the kernel reads
    want = _attn_want(held, sd, down, ws, shift)
    q_pre = F.max_pool2d(held, down, down)[n - 1, :, 0, 0] @ sd['a.qkv.weight'][:c2].double().T + sd['a.qkv.bias'][:c2].double()
    assert float(q_pre.max()) < 0 and float(F.max_pool2d(held, down, down)[0, :, 1, 0].max()) < 0  # the special cases survive the plane rounding
    from resselt_amd.archs.rha.arch import pack_hybrid

    full = {f'h.att.2.{k[2:]}': v for k, v in sd.items()}
    for k in (1, 2, 3, 4):
        full[f'h.conv.alpha{k}'] = torch.ones(1, c2, 1, 1)
    for name, ks in (('conv1x1', 1), ('conv3x3', 3), ('conv5x5', 5)):
        full[f'h.conv.{name}.weight'], full[f'h.conv.{name}.bias'] = torch.zeros(c2, 1, ks, ks), torch.zeros(c2)
    t = {k: v.to(device) for k, v in pack_hybrid(full, 'h', c2, ws).items()}
    pd = _to(pl, device)
    out = torch.full((n, c2 // 4, Hd, Wd, 4), float('nan'), device=device)
    args = lambda hi=pd.hi_ptr(off), C2=c2, dn=down, hh=H, bs=pd.batch_stride, o=out.data_ptr(): (  # noqa: E731
        hi, pd.lo_ptr(off), pd.plane_stride, bs, n, hh, W, C2, dn, ws, shift, fmt, t['wqkv_t'].data_ptr(), t['bqkv'].data_ptr(), t['pos_t'].data_ptr(),
        t['isc'].data_ptr(), t['dww'].data_ptr(), t['dwb'].data_ptr(), t['wproj_t'].data_ptr(), t['bproj'].data_ptr(), o, _stream(device))  # fmt: skip
    L.check(L.load().rsa_rha_window_attn(*args()), 'rsa_rha_window_attn')
    torch.cuda.synchronize()
    return f32map_to_nchw(out.cpu(), c2).double(), want, args, (pd, out, t)


ATTN = [  # C2, window, down, shift, batch, windows (rows, columns), plane offset
    (8, 4, 1, 0, 1, (1, 1), 0),
    (24, 4, 2, 2, 2, (2, 3), 3),
    (32, 8, 4, 4, 1, (1, 1), 1),  # Hd = Wd = window: the shifted window wraps onto itself
    (32, 8, 8, 4, 1, (2, 3), 2),
    (8, 8, 1, 4, 2, (2, 3), 1),
    (24, 8, 2, 0, 2, (1, 2), 0),
]


@pytest.mark.parametrize('c2,ws,down,shift,n,grid,off', ATTN)
def test_window_attention(device, c2, ws, down, shift, n, grid, off):
    got, want, _, _ = _attn_run(device, c2, ws, down, shift, n, grid, PF_BF16, True, off, 10 * c2 + ws + down)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'MEASURE rha_window_attn C2={c2} ws={ws} down={down} shift={shift} n={n} windows={grid}: {err:.3e} (|out|max {scale:.2f}, relative {err / scale:.2e})')
    assert not got.isnan().any()
    assert err <= 3e-5 * scale


def test_window_attention_fp16_hi_planes(device):
    got, want, _, _ = _attn_run(device, 24, 8, 2, 4, 2, (1, 2), PF_F16, False, 2, 77)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'MEASURE rha_window_attn fp16 hi planes: {err:.3e} (|out|max {scale:.2f}, relative {err / scale:.2e})')
    assert err <= 3e-5 * scale  # (the f64 formula reads the fp16 values: the output is an f32 map)


def test_window_attention_rejects_bad_arguments(device):
    _, _, args, keep = _attn_run(device, 8, 4, 2, 2, 2, (1, 1), PF_BF16, True, 1, 3)
    lib = L.load()
    pd, out, _ = keep
    assert lib.rsa_rha_window_attn(*args(C2=40)) == -1
    assert lib.rsa_rha_window_attn(*args(dn=3)) == -1
    assert lib.rsa_rha_window_attn(*args(hh=12)) == -1  # not a multiple of down * window
    assert lib.rsa_rha_window_attn(*args(bs=1)) == -1  # batch stride smaller than the planes of an image
    assert lib.rsa_rha_window_attn(*args(hi=None)) == -1
    assert lib.rsa_rha_window_attn(*args(hi=pd.hi_ptr(1) + 8)) == -3
    assert lib.rsa_rha_window_attn(*args(o=out.data_ptr() + 4)) == -3
    assert b'rha_window_attn' in lib.rsa_last_error_string()
    assert lib.rsa_rha_window_attn_lds_bytes(32, 8) == 50848 and lib.rsa_rha_window_attn_lds_bytes(8, 8) == 9544 and lib.rsa_rha_window_attn_lds_bytes(40, 8) == -1


# ------------------------------------------------------------------------------------------------------------------ mix
def _mix_run(device, c2, down, n, hw, fmt, with_lo, off, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    planes = off + c2 // 8 + 1
    x = torch.randn((n, planes * 8, H, W), generator=g)
    att = torch.randn((n, c2, H // down, W // down), generator=g)
    w, b = torch.randn((c2, 1, 5, 5), generator=g) / 5, torch.randn(c2, generator=g) * 0.2
    pl = nchw_to_planes(x, with_lo, fmt)
    held = planes_to_nchw(pl, planes * 8)[:, 8 * off : 8 * off + c2].double()
    up = F.interpolate(att.double(), scale_factor=down, mode='bilinear', align_corners=False) if down > 1 else att.double()
    want = torch.cat((F.conv2d(held, w.double(), b.double(), padding=2, groups=c2), up), 1)
    pd = _to(pl, device)
    am = nchw_to_f32map(att).to(device)
    out = Planes.empty(n, c2 // 4, H, W, device, with_lo, fmt)
    wd, bd = w.reshape(c2, 25).contiguous().to(device), b.to(device)
    args = lambda hi=pd.hi_ptr(off), dn=down, ohi=out.hi_ptr(), a=am.data_ptr(): (  # noqa: E731
        hi, pd.lo_ptr(off), pd.plane_stride, pd.batch_stride, a, ohi, out.lo_ptr(), out.plane_stride, out.batch_stride, n, H, W, c2, dn, fmt, wd.data_ptr(),
        bd.data_ptr(), _stream(device))  # fmt: skip
    L.check(L.load().rsa_rha_mix(*args()), 'rsa_rha_mix')
    torch.cuda.synchronize()
    got = planes_to_nchw(Planes(out.hi.cpu(), out.lo.cpu() if with_lo else None), 2 * c2).double()
    return got, want, args, (pd, am, out, wd, bd)


@pytest.mark.parametrize('c2,down,n,hw,off', [(8, 1, 2, (9, 35), 1), (16, 2, 1, (18, 66), 0), (32, 4, 1, (12, 40), 2), (24, 8, 2, (16, 72), 1), (8, 2, 1, (2, 2), 0)])
def test_mix(device, c2, down, n, hw, off):
    got, want, _, _ = _mix_run(device, c2, down, n, hw, PF_BF16, True, off, c2 + down)
    scale = want.abs().max().item()
    e1, e2 = (got[:, :c2] - want[:, :c2]).abs().max().item(), (got[:, c2:] - want[:, c2:]).abs().max().item()
    print(f'MEASURE rha_mix C2={c2} down={down} n={n} map={hw}: conv {e1:.3e}, upsample {e2:.3e} (|out|max {scale:.2f})')
    assert max(e1, e2) <= (2.0**-17 + 4e-6) * scale


def test_mix_fp16_hi_planes(device):
    got, want, _, _ = _mix_run(device, 16, 4, 1, (12, 36), PF_F16, False, 1, 5)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'MEASURE rha_mix fp16 hi planes: {err:.3e} (|out|max {scale:.2f})')
    assert err <= (2.0**-11 + 4e-6) * scale


def test_mix_rejects_bad_arguments(device):
    _, _, args, keep = _mix_run(device, 8, 2, 1, (4, 6), PF_BF16, True, 0, 9)
    lib = L.load()
    pd = keep[0]
    assert lib.rsa_rha_mix(*args(dn=3)) == -1
    assert lib.rsa_rha_mix(*args(dn=4)) == -1  # 6 is not a multiple of 4
    assert lib.rsa_rha_mix(*args(a=None)) == -1
    assert lib.rsa_rha_mix(*args(ohi=pd.hi_ptr())) == -1  # in place
    assert lib.rsa_rha_mix(*args(hi=pd.hi_ptr() + 8)) == -3
    assert b'rha_mix' in lib.rsa_last_error_string()


# ------------------------------------------------------------------------------------------------------------------ gate
def _gate_run(device, hp, ip, n, hw, fmt, with_lo, seed):
    g = torch.Generator().manual_seed(seed)
    cp = hp - ip
    f = torch.randn((n, 16 * hp, *hw), generator=g) * 2
    a = torch.randn((n, 8 * cp, *hw), generator=g)
    f[0, 0, 0, 0], f[0, 1, 0, 0] = 30.0, -30.0  # both tails of mish
    fp, ap = nchw_to_planes(f, with_lo, fmt), nchw_to_planes(a, with_lo, fmt)
    fh, ah = planes_to_nchw(fp, 16 * hp).double(), planes_to_nchw(ap, 8 * cp).double()
    gg, i, c = fh[:, : 8 * hp], fh[:, 8 * hp : 8 * (hp + ip)], fh[:, 8 * (hp + ip) :]
    want = F.mish(gg) * torch.cat((i, ah * c), 1)
    fd, ad = _to(fp, device), _to(ap, device)
    out = Planes.empty(n, hp, *hw, device, with_lo, fmt)
    args = lambda hi=fd.hi_ptr(), ipl=ip, ohi=out.hi_ptr(): (  # noqa: E731
        hi, fd.lo_ptr(), fd.plane_stride, fd.batch_stride, ad.hi_ptr(), ad.lo_ptr(), ad.plane_stride, ad.batch_stride, ohi, out.lo_ptr(), out.plane_stride,
        out.batch_stride, n, hw[0], hw[1], hp, ipl, fmt, _stream(device))  # fmt: skip
    L.check(L.load().rsa_rha_gate(*args()), 'rsa_rha_gate')
    torch.cuda.synchronize()
    got = planes_to_nchw(Planes(out.hi.cpu(), out.lo.cpu() if with_lo else None), 8 * hp).double()
    return got, want, args, (fd, ad, out)


@pytest.mark.parametrize('hp,ip,n,hw', [(6, 2, 2, (5, 7)), (4, 0, 1, (5, 7)), (3, 1, 1, (17, 19))])
def test_gate(device, hp, ip, n, hw):
    got, want, _, _ = _gate_run(device, hp, ip, n, hw, PF_BF16, True, 10 * hp + ip)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'MEASURE rha_gate hidden planes {hp}, i planes {ip}, map={hw}: {err:.3e} (|out|max {scale:.2f})')
    assert err <= 1e-5 * scale


def test_gate_fp16_hi_planes(device):
    got, want, _, _ = _gate_run(device, 4, 2, 1, (5, 7), PF_F16, False, 4)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f'MEASURE rha_gate fp16 hi planes: {err:.3e} (|out|max {scale:.2f})')
    assert err <= (2.0**-11 + 1e-6) * scale


def test_gate_rejects_bad_arguments(device):
    _, _, args, keep = _gate_run(device, 4, 2, 1, (5, 7), PF_BF16, True, 8)
    lib = L.load()
    fd = keep[0]
    assert lib.rsa_rha_gate(*args(ipl=4)) == -1  # no c planes left
    assert lib.rsa_rha_gate(*args(ipl=-1)) == -1
    assert lib.rsa_rha_gate(*args(hi=None)) == -1
    assert lib.rsa_rha_gate(*args(ohi=fd.hi_ptr())) == -1  # in place
    assert lib.rsa_rha_gate(*args(hi=fd.hi_ptr() + 8)) == -3
    assert b'rha_gate' in lib.rsa_last_error_string()
