"""GPU checks of the EIMN entry points (csrc/eimn.hip) against f64 torch on the dequantised operands, in both plane formats, with and
without lo halves.  u = 2^-24 is the unit roundoff of f32.  Every bound below is derived, none is measured.

Written format.  One unit of the written format at the value: 2^-8 (bf16 hi alone), 2^-16 (bf16 hi + lo), 2^-11 (fp16 hi alone), 2^-21 (fp16
hi + lo) relative, plus the absolute spacing 2^-24 of fp16's subnormals (as tests/test_rcan_kernels_gpu.py).

Chain.  d * u * S with d = 25 + 49 + 2 (the taps of both stages and the two bias additions: the longest dependent chain of f32 roundings
behind an output) and S the same f64 chain evaluated on |w|, |b| and |x|.  With gelu_in, x is GELU(q) and the f32 GELU adds 6 u |q| per
staged value (erff within 4 ulp of a factor <= 2, times |q| / 2, plus three roundings of the product), propagated through |w| the same way.
A border filled with the stage-1 bias, or stage 1 evaluated outside the map, misses by >= 1e-2 on these inputs.
SAL.  a = dw(x1) + b1, b = dw(x2) + b2 carry d = 10 (9 taps + bias) each; GELU has slope <= 1.13 and the f32 GELU's own error is
6 u |a|; the product adds 2 u |out|:  u * (10 * (1.13 * Sa * |b| + |GELU(a)| * Sb) + 6 |a| |b| + 2 |out|).
Multiply.  d = 1: u * |silu(f)| |v|.
DFFM reduce.  Sums within RSA_EIMN_DFFM_DEPTH * u * sum|v|, the depth stated in the kernel source (each value rounded to f32 once, six
butterfly levels, three additions of wave partials: 10).  Gates: 4 u from the same sums (f64 inside, one rounding to f32; a sigmoid is at
most 1, |s_g| < 4 on these weights).
DFFM apply.  First-order propagation of the f32 roundings of a C-term mean, a C-term variance, the C-term dot products of local_reduce and
the rc-term spatial gate (``_apply_bound``), through the stage LayerNorm when it runs; the planes add one unit of the written format.
"""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import eimn_oracle as O
from resselt_amd.archs.eimn.arch import _half_planes, query_layout
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops, tensors
from resselt_amd.engine.tensors import PF_BF16, PF_F16

pytestmark = pytest.mark.gpu

U = 2.0**-24
DEPTH = 10  # RSA_EIMN_DFFM_DEPTH (include/resselt_amd.h; csrc/eimn.hip, dffm_reduce_kernel)
E_ARG, E_ALIGN = -1, -3
FORMATS = [(PF_BF16, True), (PF_BF16, False), (PF_F16, True), (PF_F16, False)]
BITS = {(PF_BF16, False): 8, (PF_BF16, True): 16, (PF_F16, False): 11, (PF_F16, True): 21}
TILE_W, TILE_H = 32, 16  # csrc/eimn.hip, EQ_TW x EQ_TH


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def _unit(want, fmt, with_lo):
    return 2.0 ** -BITS[(fmt, with_lo)] * want.abs() + (2.0**-24 if fmt == PF_F16 else 2.0**-60)


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _planes(x, device, fmt, with_lo):
    """(device planes, their dequantised f64 value on the host)."""
    p = tensors.nchw_to_planes(x.float().to(device), with_lo=with_lo, fmt=fmt)
    return p, tensors.planes_to_nchw(p, x.shape[1]).cpu().double()


def _close(got, want, bound, what):
    ratio = ((got - want).abs() / bound).max().item()
    print(f'{what}: max err / bound {ratio:.3f}')
    assert ratio <= 1.0, (what, ratio)


# ------------------------------------------------------------------------------------------------------------------ chain
CHAIN_SHAPES = [(1, 64, 5, 7), (2, 64, 9, 33), (1, 48, 13, 10), (1, 64, 17, 70), (1, 64, TILE_H, TILE_W), (1, 64, TILE_H + 1, TILE_W + 1)]


def _chain_case(n, dim, h, w, seed):
    """Operands in the kernel's padded layout (dim 48: groups 18 / 6 / 24 re-laid to 3 + 1 + 3 planes, zeros in the gaps)."""
    perm, planes, (c1, c2, c3) = query_layout(dim)
    cp = 8 * sum(planes)
    idx = torch.tensor(perm)
    q, w1, b1, w2, b2 = (torch.zeros(s, dtype=torch.float64) for s in ((n, cp, h, w), (cp, 25), (cp,), (cp, 49), (cp,)))
    q[:, idx] = _rand((n, dim, h, w), seed, 4.0)
    w1[idx], b1[idx] = _rand((dim, 25), seed + 1, 0.3), _rand((dim,), seed + 2, 0.5)
    w2[idx[:c1], :25], b2[idx[:c1]] = _rand((c1, 25), seed + 3, 0.3), _rand((c1,), seed + 4, 0.5)
    w2[idx[c1 + c2 :]], b2[idx[c1 + c2 :]] = _rand((c3, 49), seed + 5, 0.2), _rand((c3,), seed + 6, 0.5)
    return q, [t.float().double() for t in (w1, b1, w2, b2)], planes  # the weights as the f32 values the kernel reads


def _chain_bound(qq, w1, b1, w2, b2, planes, gelu, want, fmt, with_lo):
    staged = F.gelu(qq).abs() if gelu else qq.abs()
    bound = _unit(want, fmt, with_lo) + (25 + 49 + 2) * U * O.chain_f64(staged, w1.abs(), b1.abs(), w2.abs(), b2.abs(), planes, gelu=False)
    if gelu:
        zero = torch.zeros_like(b1)
        bound = bound + 6 * U * O.chain_f64(qq.abs(), w1.abs(), zero, w2.abs(), zero, planes, gelu=False)
    return bound


@pytest.mark.parametrize('gelu', [True, False])
@pytest.mark.parametrize('fmt,with_lo', FORMATS)
@pytest.mark.parametrize('n,dim,h,w', CHAIN_SHAPES)
def test_query_chain(device, n, dim, h, w, fmt, with_lo, gelu):
    q, (w1, b1, w2, b2), planes = _chain_case(n, dim, h, w, 17 * h + w)
    cp = q.shape[1]
    qp, qq = _planes(q, device, fmt, with_lo)
    out = tensors.Planes.empty(n, cp // 8, h, w, device, with_lo=with_lo, fmt=fmt)
    out.hi.fill_(float('nan'))
    dv = [_half_planes(w1).to(device), b1.float().to(device), _half_planes(w2).to(device), b2.float().to(device)]
    L.check(L.load().rsa_eimn_query_chain(qp.hi_ptr(), qp.lo_ptr(), qp.plane_stride, qp.batch_stride, out.hi_ptr(), out.lo_ptr(), out.plane_stride,
                                          out.batch_stride, n, h, w, *planes, int(gelu), fmt, *(t.data_ptr() for t in dv), _stream(device)), 'chain')  # fmt: skip
    torch.cuda.synchronize()
    got = tensors.planes_to_nchw(out, cp).cpu().double()
    want = O.chain_f64(qq, w1, b1, w2, b2, planes, gelu=gelu)
    bound = _chain_bound(qq, w1, b1, w2, b2, planes, gelu, want, fmt, with_lo)
    assert bool(torch.isfinite(got).all())  # every unit of the output was written
    _close(got, want, bound, f'chain {n}x{dim}x{h}x{w} fmt {fmt} lo {with_lo} gelu {gelu}')


def test_query_chain_border_is_zero_not_bias(device):
    """The property the bound protects, stated directly: with an all-zero input the first stage is its bias inside the map and 0 outside."""
    n, dim, h, w = 1, 64, 5, 7
    _, (w1, b1, w2, b2), planes = _chain_case(n, dim, h, w, 3)
    z = torch.zeros((n, dim, h, w), dtype=torch.float64)
    want = O.chain_f64(z, w1, b1, w2, b2, planes, gelu=True)
    filled = F.conv2d(b1.view(1, -1, 1, 1).expand(n, dim, h + 8, w + 8)[:, :24], w2[:24, :25].reshape(24, 1, 5, 5), b2[:24], dilation=2, groups=24)
    assert float((filled - want[:, :24]).abs().max()) >= 1e-2  # what a bias-valued halo would give
    qp, _ = _planes(z, device, PF_BF16, True)
    out = tensors.Planes.empty(n, 8, h, w, device, with_lo=True, fmt=PF_BF16)
    dv = [_half_planes(w1).to(device), b1.float().to(device), _half_planes(w2).to(device), b2.float().to(device)]
    L.check(L.load().rsa_eimn_query_chain(qp.hi_ptr(), qp.lo_ptr(), qp.plane_stride, qp.batch_stride, out.hi_ptr(), out.lo_ptr(), out.plane_stride,
                                          out.batch_stride, n, h, w, *planes, 1, PF_BF16, *(t.data_ptr() for t in dv), _stream(device)), 'chain')  # fmt: skip
    torch.cuda.synchronize()
    got = tensors.planes_to_nchw(out, dim).cpu().double()
    _close(got, want, _chain_bound(z, w1, b1, w2, b2, planes, True, want, PF_BF16, True), 'chain on zeros')


# ------------------------------------------------------------------------------------------------------------------ SAL, multiply
@pytest.mark.parametrize('fmt,with_lo', FORMATS)
@pytest.mark.parametrize('n,c,h,w', [(1, 16, 5, 7), (2, 24, 9, 33), (1, 128, 17, 70)])
def test_sal(device, n, c, h, w, fmt, with_lo):
    x = _rand((n, 2 * c, h, w), 5 * h + w, 4.0)
    wt, b = _rand((2 * c, 9), 1, 0.4).float().double(), _rand((2 * c,), 2, 0.5).float().double()
    xp, xq = _planes(x, device, fmt, with_lo)
    out = tensors.Planes.empty(n, c // 8, h, w, device, with_lo=with_lo, fmt=fmt)
    wd, bd = wt.float().to(device), b.float().to(device)
    L.check(L.load().rsa_eimn_sal(xp.hi_ptr(), xp.lo_ptr(), xp.plane_stride, xp.batch_stride, out.hi_ptr(), out.lo_ptr(), out.plane_stride, out.batch_stride,
                                  n, h, w, c // 8, fmt, wd.data_ptr(), bd.data_ptr(), _stream(device)), 'sal')  # fmt: skip
    torch.cuda.synchronize()
    got = tensors.planes_to_nchw(out, c).cpu().double()
    a, bb = F.conv2d(xq, wt.reshape(2 * c, 1, 3, 3), b, padding=1, groups=2 * c).chunk(2, dim=1)
    sa, sb = F.conv2d(xq.abs(), wt.abs().reshape(2 * c, 1, 3, 3), b.abs(), padding=1, groups=2 * c).chunk(2, dim=1)
    want = F.gelu(a) * bb
    assert torch.equal(want, O.sal_f64(xq, wt, b))
    bound = _unit(want, fmt, with_lo) + U * (10 * (1.13 * sa * bb.abs() + F.gelu(a).abs() * sb) + 6 * a.abs() * bb.abs() + 2 * want.abs())
    _close(got, want, bound, f'sal {n}x{c}x{h}x{w} fmt {fmt} lo {with_lo}')


@pytest.mark.parametrize('fmt,with_lo', FORMATS)
@pytest.mark.parametrize('n,c,h,w', [(2, 48, 5, 7), (1, 64, 17, 70)])
def test_silu_mul(device, n, c, h, w, fmt, with_lo):
    f, v = _rand((n, c, h, w), 3, 6.0), _rand((n, c, h, w), 4, 4.0)
    fp, fq = _planes(f, device, fmt, with_lo)
    vp, vq = _planes(v, device, fmt, with_lo)
    out = tensors.Planes.empty(n, c // 8, h, w, device, with_lo=with_lo, fmt=fmt)

    def call(dst):
        L.check(L.load().rsa_eimn_silu_mul(fp.hi_ptr(), fp.lo_ptr(), fp.plane_stride, fp.batch_stride, vp.hi_ptr(), vp.lo_ptr(), vp.plane_stride,
                                           vp.batch_stride, dst.hi_ptr(), dst.lo_ptr(), dst.plane_stride, dst.batch_stride, n, h, w, c // 8, fmt,
                                           _stream(device)), 'silu_mul')  # fmt: skip
        torch.cuda.synchronize()

    call(out)
    want = fq * torch.sigmoid(fq) * vq
    got = tensors.planes_to_nchw(out, c).cpu().double()
    _close(got, want, _unit(want, fmt, with_lo) + 1 * U * want.abs(), f'silu_mul {n}x{c}x{h}x{w} fmt {fmt} lo {with_lo}')
    call(fp)  # in place over f, as the plan runs it
    assert torch.equal(fp.hi, out.hi) and (not with_lo or torch.equal(fp.lo, out.lo))


# ------------------------------------------------------------------------------------------------------------------ DFFM
DFFM_SHAPES = [(2, 64, 5, 7), (1, 48, 9, 130), (1, 64, 37, 53)]


def _dffm_weights(c, seed):
    rc = c // 4
    f = dict(gamma=1.0 + _rand((c,), seed, 0.5), beta=_rand((c,), seed + 1, 0.3), wg=_rand((rc, c), seed + 2, 1.5 / c**0.5), bg=_rand((rc,), seed + 3, 0.3),
             wl=_rand((rc, c), seed + 4, 1.5 / c**0.5), bl=_rand((rc,), seed + 5, 0.3), wc=_rand((c, rc), seed + 6, 1.5 / rc**0.5), bc=_rand((c,), seed + 7, 0.3),
             ws=_rand((2 * rc,), seed + 8, 1.0 / rc**0.5), bs=_rand((1,), seed + 9, 0.3), ls2=0.35 + _rand((c,), seed + 10, 0.25))  # fmt: skip
    return {k: v.float().double() for k, v in f.items()}  # the f32 values the kernels read


def _reduce(device, z_map, n, c, h, w, f, fill):
    lib = L.load()
    nbytes = int(lib.rsa_eimn_dffm_workspace_bytes(n, h, w, c))
    slots = -(-h * w // 256)
    assert nbytes == n * slots * c * 4
    work = torch.full((n, slots, c), fill, dtype=torch.float32, device=device)
    g, b = f['gamma'].float().to(device), f['beta'].float().to(device)
    L.check(lib.rsa_eimn_dffm_reduce(z_map.data_ptr(), n, h, w, c, g.data_ptr(), b.data_ptr(), 1e-6, work.data_ptr(), nbytes, _stream(device)), 'dffm_reduce')
    torch.cuda.synchronize()
    return work, nbytes


def _gates(device, work, nbytes, n, c, h, w, f):
    rc = c // 4
    dv = [f[k].float().to(device).contiguous() for k in ('wg', 'bg', 'wc', 'bc', 'ws', 'bs')]
    gates = torch.full((n, c + 4), float('nan'), dtype=torch.float32, device=device)
    L.check(L.load().rsa_eimn_dffm_gates(work.data_ptr(), nbytes, n, h, w, c, rc, *(t.data_ptr() for t in dv), gates.data_ptr(), _stream(device)), 'dffm_gates')
    torch.cuda.synchronize()
    return gates


@pytest.mark.parametrize('n,c,h,w', DFFM_SHAPES)
def test_dffm_reduce_and_gates(device, n, c, h, w):
    f = _dffm_weights(c, 7 * c + h)
    z = (_rand((n, c, h, w), 11, 3.0) + _rand((1, c, 1, 1), 12, 1.0)).float()
    z_map = tensors.nchw_to_f32map(z.to(device))
    work, nbytes = _reduce(device, z_map, n, c, h, w, f, float('nan'))
    again, _ = _reduce(device, z_map, n, c, h, w, f, -1.0)
    assert bool(torch.isfinite(work).all())  # every workspace entry is written
    assert torch.equal(work, again)  # a fixed order: bit for bit, whatever the buffer held
    v = O.layernorm_cf(z.double(), f['gamma'], f['beta'])
    want = v.sum(dim=(2, 3))
    got = work.cpu().double().sum(dim=1)
    _close(got, want, DEPTH * U * v.abs().sum(dim=(2, 3)), f'dffm sums {n}x{c}x{h}x{w}')
    gates = _gates(device, work, nbytes, n, c, h, w, f).cpu().double()
    c_attn, s_g = O.dffm_gates_f64(got / (h * w), f)
    assert float(s_g.abs().max()) < 4.0  # the absolute bound below covers the final rounding of s_g only below 4
    gerr = max((gates[:, :c] - c_attn).abs().max().item(), (gates[:, c] - s_g).abs().max().item())
    print(f'dffm gates {n}x{c}x{h}x{w}: err {gerr:.3e}')
    assert gerr <= 4 * U and float(gates[:, c + 1 :].abs().max()) == 0.0


def _ln_bound(v, dv, gamma, beta, eps):
    """First-order bound of an f32 LayerNorm over dim 1 of f64 values ``v`` known to within ``dv``: (value, bound)."""
    c = v.shape[1]
    mu = v.mean(1, keepdim=True)
    dmu = dv.mean(1, keepdim=True) + c * U * v.abs().mean(1, keepdim=True)  # a C-term f32 sum
    d = v - mu
    dd = dv + dmu + U * d.abs()
    var = d.pow(2).mean(1, keepdim=True)
    dvar = (c + 2) * U * var + 2 * (d.abs() * dd).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    rel_r = 0.5 * dvar / (var + eps) + 3 * U  # the addition of eps, the square root, the division
    g = gamma[None, :, None, None]
    out = g * d * r + beta[None, :, None, None]
    return out, g.abs() * r * (dd + d.abs() * (rel_r + 2 * U)) + U * out.abs()


def _apply_bound(z, x, c_attn, s_g, f, norm, add):
    """First-order bound of rsa_eimn_dffm_apply's f32 arithmetic, operation by operation (module docstring)."""
    c, rc = z.shape[1], f['wl'].shape[0]
    nrm, dn = _ln_bound(z, torch.zeros_like(z), f['gamma'], f['beta'], 1e-6)
    wl = f['wl'].abs()
    lin = torch.einsum('rc,nchw->nrhw', f['wl'], nrm) + f['bl'][None, :, None, None]
    dl = torch.einsum('rc,nchw->nrhw', wl, dn) + (c + 1) * U * (torch.einsum('rc,nchw->nrhw', wl, nrm.abs()) + f['bl'].abs()[None, :, None, None])
    gl = F.gelu(lin)
    dgl = 1.13 * dl + 6 * U * lin.abs()
    ws = f['ws'][:rc].abs()
    pre_abs = s_g.abs()[:, None, None] + torch.einsum('r,nrhw->nhw', ws, gl.abs())
    dpre = torch.einsum('r,nrhw->nhw', ws, dgl) + (rc + 1) * U * pre_abs
    s = torch.sigmoid(torch.einsum('r,nrhw->nhw', f['ws'][:rc], gl) + s_g[:, None, None])
    ds = 0.25 * dpre + 4 * U * s
    kz = (f['ls2'][None, :, None, None] * c_attn[:, :, None, None] * z).abs()
    v = x + f['ls2'][None, :, None, None] * c_attn[:, :, None, None] * z * s[:, None]
    dv = kz * ds[:, None] + 4 * U * kz * s[:, None] + U * v.abs()
    if norm is not None:
        v, dv = _ln_bound(v, dv, norm[0], norm[1], norm[2])
    if add is not None:
        v = v + add
        dv = dv + U * v.abs()
    return dv


@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('with_norm', [False, True])
@pytest.mark.parametrize('fmt,with_lo', FORMATS)
@pytest.mark.parametrize('n,c,h,w', DFFM_SHAPES)
def test_dffm_apply(device, n, c, h, w, fmt, with_lo, with_norm, with_add):
    lib = L.load()
    rc = c // 4
    f = _dffm_weights(c, 3 * c + w)
    z = (_rand((n, c, h, w), 21, 3.0) + _rand((1, c, 1, 1), 22, 1.0)).float()
    x = _rand((n, c, h, w), 23, 2.0).float()
    add = _rand((n, c, h, w), 24, 1.0).float() if with_add else None
    ng, nb = (1.0 + _rand((c,), 25, 0.5)).float(), _rand((c,), 26, 0.3).float()
    z_map, x_map = tensors.nchw_to_f32map(z.to(device)), tensors.nchw_to_f32map(x.to(device))
    add_map = tensors.nchw_to_f32map(add.to(device)) if with_add else None
    work, nbytes = _reduce(device, z_map, n, c, h, w, f, 0.0)
    gates = _gates(device, work, nbytes, n, c, h, w, f)
    dv = {k: f[k].float().to(device).contiguous() for k in ('gamma', 'beta', 'wl', 'bl', 'ws', 'ls2')}
    ngd, nbd = ng.to(device), nb.to(device)
    out32 = torch.full_like(x_map, float('nan'))
    out = tensors.Planes.empty(n, c // 8, h, w, device, with_lo=with_lo, fmt=fmt)

    def call(dst32):
        L.check(lib.rsa_eimn_dffm_apply(z_map.data_ptr(), x_map.data_ptr(), n, h, w, c, rc, dv['gamma'].data_ptr(), dv['beta'].data_ptr(), 1e-6, dv['wl'].data_ptr(),
                                        dv['bl'].data_ptr(), dv['ws'].data_ptr(), gates.data_ptr(), dv['ls2'].data_ptr(), ngd.data_ptr() if with_norm else None,
                                        nbd.data_ptr() if with_norm else None, 1e-5, add_map.data_ptr() if with_add else None, dst32.data_ptr(), out.hi_ptr(),
                                        out.lo_ptr(), out.plane_stride, out.batch_stride, fmt, _stream(device)), 'dffm_apply')  # fmt: skip
        torch.cuda.synchronize()

    call(out32)
    gh = gates.cpu().double()
    norm = (ng.double(), nb.double(), 1e-5) if with_norm else None
    args = (z.double(), x.double(), gh[:, :c], gh[:, c], f)
    want = O.dffm_apply_f64(*args, norm=norm, add=add.double() if with_add else None)
    bound = _apply_bound(*args, norm, add.double() if with_add else None)
    tag = f'dffm apply {n}x{c}x{h}x{w} fmt {fmt} lo {with_lo} norm {with_norm} add {with_add}'
    _close(tensors.f32map_to_nchw(out32, c).cpu().double(), want, bound + 2.0**-60, tag + ' f32')
    _close(tensors.planes_to_nchw(out, c).cpu().double(), want, bound + _unit(want, fmt, with_lo), tag + ' planes')
    first_hi, first32 = out.hi.clone(), out32.clone()
    call(x_map)  # in place over the stream, as a plan may run it
    assert torch.equal(x_map, first32) and torch.equal(out.hi, first_hi)


def test_argument_checks(device):
    """Each refusal returns its documented code and launches nothing: the outputs keep their sentinel."""
    lib = L.load()
    n, c, h, w, rc = 1, 64, 8, 8, 16
    z = torch.zeros(8192, dtype=torch.float32, device=device)
    sent = torch.full((8192,), 7.0, dtype=torch.float32, device=device)
    p, o = z.data_ptr(), sent.data_ptr()
    nbytes = int(lib.rsa_eimn_dffm_workspace_bytes(n, h, w, c))
    assert nbytes == 64 * 4 and lib.rsa_eimn_dffm_workspace_bytes(n, h, w, 60) == E_ARG and lib.rsa_eimn_dffm_workspace_bytes(n, h, w, 136) == E_ARG

    def reduce(c=c, work=o, zp=p):
        return lib.rsa_eimn_dffm_reduce(zp, n, h, w, c, p, p, 1e-6, work, nbytes, None)

    def gates(c=c, rc=rc, work=p, out=o):
        return lib.rsa_eimn_dffm_gates(work, nbytes, n, h, w, c, rc, p, p, p, p, p, p, out, None)

    def apply(c=c, rc=rc, out32=o, hi=o + 4096, zp=p):
        return lib.rsa_eimn_dffm_apply(zp, p, n, h, w, c, rc, p, p, 1e-6, p, p, p, p, p, None, None, 1e-5, None, out32, hi, None, 64, 512, 0, None)

    def chain(planes=(3, 1, 4), qp=p, out=o):
        return lib.rsa_eimn_query_chain(qp, None, 64, 512, out, None, 64, 512, n, h, w, *planes, 1, 0, p, p, p, p, None)

    def sal(planes=2, xp=p, out=o):
        return lib.rsa_eimn_sal(xp, None, 64, 512, out, None, 64, 512, n, h, w, planes, 0, p, p, None)

    # dim not a multiple of 8
    assert reduce(c=60) == E_ARG and gates(c=60) == E_ARG and apply(c=60) == E_ARG
    # rc > 32
    assert gates(rc=33) == E_ARG and apply(rc=33) == E_ARG and gates(rc=0) == E_ARG
    # a misaligned pointer
    assert reduce(zp=p + 8) == E_ALIGN and reduce(work=o + 4) == E_ALIGN and gates(out=o + 8) == E_ALIGN and apply(hi=o + 4096 + 8) == E_ALIGN
    assert chain(qp=p + 8) == E_ALIGN and sal(out=o + 8) == E_ALIGN
    # a null workspace
    assert reduce(work=None) == E_ARG and gates(work=None) == E_ARG
    # the rest of the documented refusals
    assert chain(planes=(0, 0, 0)) == E_ARG and chain(out=p) == E_ARG and sal(planes=0) == E_ARG and sal(out=p) == E_ARG
    assert lib.rsa_eimn_dffm_reduce(p, n, h, w, c, p, p, 1e-6, o, nbytes - 4, None) == E_ARG  # a workspace that is too small
    # a batch stride smaller than an image's planes (two images would overlap)
    assert lib.rsa_eimn_query_chain(p, None, 64, 8 * 64 - 1, o, None, 64, 512, 2, h, w, 3, 1, 4, 1, 0, p, p, p, p, None) == E_ARG
    assert lib.rsa_eimn_sal(p, None, 64, 4 * 64 - 1, o, None, 64, 512, 2, h, w, 2, 0, p, p, None) == E_ARG
    assert lib.rsa_eimn_silu_mul(p, None, 64, 512, p, None, 64, 512, o, None, 64, 8 * 64 - 1, 2, h, w, 8, 0, None) == E_ARG
    assert lib.rsa_eimn_dffm_apply(p, p, 2, h, w, c, rc, p, p, 1e-6, p, p, p, p, p, None, None, 1e-5, None, o, o + 16384, None, 64, 8 * 64 - 1, 0, None) == E_ARG
    torch.cuda.synchronize()
    assert float((sent - 7.0).abs().max()) == 0.0 and float(z.abs().max()) == 0.0  # nothing was launched
    assert lib.rsa_last_error_string()
