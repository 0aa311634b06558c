"""fp64 references, derived forward-error bounds, float32 emulations and the case list of the per-token normalisation kernels
(rsa_layernorm, rsa_layernorm_gelu, rsa_rmsnorm).  A plain helper module: tests/test_norm_reference.py checks on the CPU that the bounds
mean something, tests/test_norm_kernels_gpu.py holds the kernels to them.  Every function works on NCHW tensors of any device.

Notation.  One token = the C channels x_c of one pixel.  In f64: m = mean_c x_c, d_c = x_c - m, var = mean_c d_c^2,
sigma = sqrt(var + eps) (so a constant pixel, var = 0, stays bounded), n_c = d_c / sigma, v_c = n_c g_c + b_c.
A1 = mean_c |x_c|.  u = 2^-24 is the unit roundoff of f32; a library function documented at k ulp is within 2 k u relative.

LayerNorm (csrc/swin.hip, all four kernels; first order in u, magnitudes from the f64 intermediates of the token):

  mean      C - 1 additions in any order (every partial sum is at most sum |x_c|), the product by a rounded 1 / C:
                |dm| <= (C - 1) u A1 + 2 u |m| <= (C + 1) u A1                                                       =: dm
  d_c       the deviations are centred, one subtraction each: computed d_c = d_c - dm' + rho_c with one shared shift |dm'| <= dm and
            |rho_c| <= u |d_c|:                                                                        dd_c = dm + u |d_c|
  var       sum_c (d_c - dm')^2 = sum_c d_c^2 + C dm'^2 because sum_c d_c = 0: the shared shift enters the variance at second order
            only.  What is left at first order: the squares and their C - 1 additions (C multiply-adds; (C + 1) u if they are not
            fused), the product by the rounded 1 / C (2 u), and rho_c twice (2 u):        |d var| <= (C + 5) u var
  rstd      the addition of eps (u), the square root halves the relative error, rsqrtf within 1 ulp (HIP's documented accuracy):
                rr = ((C + 5) / 2 + 1 + 2) u            (var / sigma^2 <= 1)
  n_c       one product:                                 |dn_c| <= dd_c / sigma + |n_c| (rr + u)       <- the conditioning: A1 / sigma
  v_c       one multiply-add with g_c and b_c (two roundings if not fused):
                                                         |dv_c| <= |g_c| |dn_c| + u (|n_c g_c| + |v_c|)
  The `v * rstd + nm` form (nm = -mean * rstd rounded once, then one fused multiply-add per channel) adds the rounding of nm:
                                                         + u |m| / sigma |g_c|                           (form = 'nm')

Second order.  Every relative quantity above is at most E = dm / sigma + rr per token; the terms the derivation drops are products of two of
them (dm'^2 / sigma^2 in the variance: E^2 / 2 in rstd; dn times rr; ...), at most four such products per element, so they are covered by the
factor SECOND = 1 + 4 E_MAX = 1.25 with E_MAX = 2^-4.  `max_e` returns E and the CPU test asserts E <= E_MAX for every listed case; nothing else
enters the factor.

GELU(LayerNorm) (csrc/rgt.hip: one thread per pixel; mean = sum / C, C fused multiply-adds for the variance, 1 / sqrtf).  The same counts
hold with the division (1 ulp) and sqrtf (1 ulp) in place of rsqrtf: ROOT_U = 4 instead of 2.  z = 0.5 a (1 + erf(a / sqrt 2)) of a = v_c:
|gelu'| <= 1.13; the scaled argument carries 2 u and t erf'(t) <= 0.5; erff is within 4 ulp (HIP's documented accuracy) of a value in
[-1, 1], at most 8 u absolute; 1 + erf is one addition of a value <= 2; so 1 + erf is within 11 u absolute and
                                                         |dz| <= 1.13 |da| + 5.5 u |a| + u |z|

RMSNorm (csrc/rtmosr.hip: scale x / (||x||_2 C^-1/2 + eps) + offset).  ss = sum x_c^2, positive terms: (C + 1) u relative; sqrtf halves
it and adds 2 u; rsqrtf((float)C) 2 u; their product u; D = rms + eps one addition (u, and rms / D <= 1); 1 / D one division (2 u):
                ri = ((C + 1) / 2 + 8) u relative on inv = 1 / D
  y_c = scale_c (x_c inv) + offset_c   a product and a multiply-add:
                                                         |dy_c| <= |s_c x_c / D| (ri + 2 u) + u |y_c|
A pixel of zeros gives ss = 0, inv = 1 / eps (finite), y_c = offset_c exactly.  SECOND covers its second order as well (ri <= E_MAX).

Plane formats (`plane_term`, added per element on |ref|): 2^-17 bf16 hi + lo, 2^-8 bf16 hi, 2^-11 fp16 hi (the project's values, see
tests/test_flexnet_kernels_gpu.py), 2^-22 fp16 hi + lo plus 2^-25 absolute for fp16's subnormal grid, nothing for the f32 map.

Nothing here is fitted to what a GPU returns.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

U = 2.0**-24
E_MAX = 2.0**-4
SECOND = 1.0 + 4.0 * E_MAX
USEFUL = 2.0**-6  # a bound above USEFUL * max |ref| cannot fail anything (condition 2 of tests/test_norm_reference.py)
PF_BF16, PF_F16 = 0, 1  # enum rsa_plane_fmt


def _cv(t, ref):
    return t.to(device=ref.device, dtype=torch.float64).reshape(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ f64 references
def ln_stats(x: torch.Tensor, eps: float):
    """f64 (m, d, sigma) of an NCHW tensor, per token."""
    xd = x.double()
    m = xd.mean(1, keepdim=True)
    d = xd - m
    return m, d, ((d * d).mean(1, keepdim=True) + eps).sqrt()


def layernorm_ref(x, gamma, beta, eps):
    m, d, sigma = ln_stats(x, eps)
    return d / sigma * _cv(gamma, d) + _cv(beta, d)


def gelu_ref(a):
    return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))


def layernorm_gelu_ref(x, gamma, beta, eps):
    return gelu_ref(layernorm_ref(x, gamma, beta, eps))


def rmsnorm_ref(x, scale, offset, eps):
    xd = x.double()
    rms = (xd * xd).sum(1, keepdim=True).sqrt() * xd.shape[1] ** -0.5
    return _cv(scale, xd) * (xd / (rms + eps)) + _cv(offset, xd)


# ------------------------------------------------------------------------------------------------------------------ bounds
def max_e(x, eps, root_u: float = 2.0) -> float:
    """E of the docstring: the largest first-order relative quantity of any token."""
    C = x.shape[1]
    _, _, sigma = ln_stats(x, eps)
    dm = (C + 1) * U * x.double().abs().mean(1, keepdim=True)
    return float((dm / sigma).max()) + ((C + 5) / 2 + 1 + root_u) * U


def layernorm_bound(x, gamma, beta, eps, form: str = 'centred', root_u: float = 2.0):
    """Per-element bound on |kernel - layernorm_ref| for an f32 result.  form 'centred': (x - mean) * rstd; 'nm': x * rstd + (-mean * rstd)."""
    C = x.shape[1]
    m, d, sigma = ln_stats(x, eps)
    g, b = _cv(gamma, d), _cv(beta, d)
    n = d / sigma
    v = n * g + b
    dm = (C + 1) * U * x.double().abs().mean(1, keepdim=True)
    rr = ((C + 5) / 2 + 1 + root_u) * U
    dn = (dm + U * d.abs()) / sigma + n.abs() * (rr + U)
    dv = g.abs() * dn + U * ((n * g).abs() + v.abs())
    if form == 'nm':
        dv = dv + U * m.abs() / sigma * g.abs()
    elif form != 'centred':
        raise ValueError(form)
    return SECOND * dv


def layernorm_gelu_bound(x, gamma, beta, eps):
    a = layernorm_ref(x, gamma, beta, eps)
    da = layernorm_bound(x, gamma, beta, eps, 'centred', root_u=4.0) / SECOND
    return SECOND * (1.13 * da + 5.5 * U * a.abs() + U * gelu_ref(a).abs())


def rmsnorm_bound(x, scale, offset, eps):
    xd = x.double()
    C = xd.shape[1]
    D = (xd * xd).sum(1, keepdim=True).sqrt() * C**-0.5 + eps
    s, o = _cv(scale, xd), _cv(offset, xd)
    t = (s * xd / D).abs()
    ri = ((C + 1) / 2 + 8) * U
    return SECOND * (t * (ri + 2 * U) + U * (s * xd / D + o).abs())


def plane_term(ref, fmt, with_lo: bool):
    """What storing ref as split planes may add, per element.  fmt None: the f32 map."""
    if fmt is None:
        return torch.zeros_like(ref)
    if fmt == PF_BF16:
        return (2.0**-17 if with_lo else 2.0**-8) * ref.abs()
    return 2.0**-22 * ref.abs() + 2.0**-25 if with_lo else 2.0**-11 * ref.abs()


# ------------------------------------------------------------------------------------------------------------------ f32 emulations
def _wave_sum(t):
    """Sum over channels as the LayerNorm kernels split it: plane (8 channels) p belongs to wave p % 4; a wave adds its groups of four
    as (a + b) + (c + d) one after the other; the four partial sums are added in order.  t is f32 [N, C, H, W]."""
    n, c, h, w = t.shape
    pad = (-c) % 32
    if pad:
        t = torch.cat([t, t.new_zeros((n, pad, h, w))], 1)
    q = t.reshape(n, -1, 4, 2, 4, h, w)  # [N, k, wave, half, lane of the group, H, W]
    gs = (q[:, :, :, :, 0] + q[:, :, :, :, 1]) + (q[:, :, :, :, 2] + q[:, :, :, :, 3])  # [N, k, wave, half, H, W]
    part = t.new_zeros((n, 4, h, w))
    for k in range(gs.shape[1]):
        for hf in range(2):
            part = part + gs[:, k, :, hf]
    return (((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]).unsqueeze(1)


def emulate_layernorm(x, gamma, beta, eps, form: str = 'centred', wrong: str | None = None):
    """The kernels' arithmetic in f32 torch ops.  form 'centred' or 'nm' (both with the 4-way split of the channel sums).
    wrong: None, or one of the deliberately wrong variants 'one_pass' (E[x^2] - mean^2), 'padded_count' (divides by 4 ceil(C / 4)),
    'no_eps'."""
    x = x.float()
    C = x.shape[1]
    f = lambda t: t.to(device=x.device, dtype=torch.float32).reshape(1, -1, 1, 1)  # noqa: E731
    g, b = f(gamma), f(beta)
    count = 4 * ((C + 3) // 4) if wrong == 'padded_count' else C
    inv_c = torch.tensor(1.0, dtype=torch.float32, device=x.device) / torch.tensor(float(count), dtype=torch.float32, device=x.device)
    e = torch.tensor(0.0 if wrong == 'no_eps' else eps, dtype=torch.float32, device=x.device)
    mean = _wave_sum(x) * inv_c
    if wrong == 'one_pass':
        var = _wave_sum(x * x) * inv_c - mean * mean
    else:
        dev = x - mean
        var = _wave_sum(dev * dev) * inv_c
    rstd = torch.rsqrt(var + e)
    if form == 'nm':
        nm = -mean * rstd
        return (x * rstd + nm) * g + b
    if form != 'centred':
        raise ValueError(form)
    return (x - mean) * rstd * g + b


def emulate_layernorm_gelu(x, gamma, beta, eps):
    a = emulate_layernorm(x, gamma, beta, eps)
    return 0.5 * a * (1.0 + torch.erf(a * 0.70710678118654752440))


def emulate_rmsnorm(x, scale, offset, eps):
    x = x.float()
    C = x.shape[1]
    f = lambda t: t.to(device=x.device, dtype=torch.float32).reshape(1, -1, 1, 1)  # noqa: E731
    ss = (x * x).sum(1, keepdim=True)
    inv = 1.0 / (ss.sqrt() * torch.rsqrt(torch.tensor(float(C), dtype=torch.float32, device=x.device)) + torch.tensor(eps, dtype=torch.float32, device=x.device))
    return f(scale) * (x * inv) + f(offset)


def round_to_planes(y, fmt, with_lo: bool):
    """An f32 tensor as the split planes hold it."""
    if fmt is None:
        return y.double()
    dt = torch.float16 if fmt == PF_F16 else torch.bfloat16
    hi = y.to(dt).float()
    return (hi + (y - hi).to(dt).float()).double() if with_lo else hi.double()


# ------------------------------------------------------------------------------------------------------------------ cases
CONST_VALUE = 0.3  # the constant pixel: small enough that (C + 1) u 0.3 / sqrt(eps) stays far below E_MAX at C = 400, eps = 1e-6
MAX = 'max'  # a ratio: the largest power of two whose case still meets condition 2 (and E <= E_MAX)


@dataclass(frozen=True)
class Case:
    name: str
    op: str  # 'ln' | 'gelu' | 'rms'
    C: int
    n: int
    H: int
    W: int
    eps: float = 1e-5
    ratio: float | str = 1.0  # |offset| / sigma of the rows
    seed: int = 0
    embed: int = 0  # > 0: the first `embed` channels are the shared random ones of the three-bracket test, the rest keep mean and variance

    @property
    def tokens(self) -> int:
        return self.n * self.H * self.W


def _rows(C, n, H, W, ratio, gen):
    sig = 0.5 + torch.rand((n, 1, H, W), generator=gen, dtype=torch.float64)
    sign = torch.where(torch.rand((n, 1, H, W), generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return (ratio * sig * sign + sig * torch.randn((n, C, H, W), generator=gen, dtype=torch.float64)).float()


def _weights(C, gen):
    """gamma around 1 with every seventh channel small (0.05 x), beta around 0: small-valued channels sit beside ordinary ones, which a
    tolerance relative to the map's maximum would hide."""
    gamma = 1.0 + 0.25 * torch.randn(C, generator=gen)
    beta = 0.3 * torch.randn(C, generator=gen)
    gamma[3::7] *= 0.05
    gamma[0], beta[0] = 1.25, 0.5
    return gamma, beta


def _build(case: Case, ratio: float) -> dict:
    C = case.embed or case.C
    gen = torch.Generator().manual_seed(1000 * C + 10 * case.tokens + case.seed)
    x = _rows(C, case.n, case.H, case.W, ratio, gen)
    gamma, beta = _weights(C, gen)
    const_tok = zero_tok = None
    if case.tokens >= 8 and not case.embed:
        const_tok, zero_tok = (case.n - 1, case.H - 1, case.W - 1), (0, 0, case.W // 2)
        x[const_tok[0], :, const_tok[1], const_tok[2]] = CONST_VALUE
        x[zero_tok[0], :, zero_tok[1], zero_tok[2]] = 0.0
    if case.embed and case.C > C:
        # the extra channels: m +- s alternately (an even count), which keeps the token's mean and variance; gamma = beta = 0 there
        extra = case.C - C
        assert extra % 2 == 0
        xd = x.double()
        m = xd.mean(1, keepdim=True)
        s = ((xd - m) ** 2).mean(1, keepdim=True).sqrt()
        alt = torch.where(torch.arange(extra) % 2 == 0, 1.0, -1.0).reshape(1, extra, 1, 1).double()
        x = torch.cat([x, (m + alt * s).float()], 1)
        gamma, beta = torch.cat([gamma, torch.zeros(extra)]), torch.cat([beta, torch.zeros(extra)])
    return dict(x=x, gamma=gamma, beta=beta, eps=case.eps, const_tok=const_tok, zero_tok=zero_tok, ratio=ratio)


def reference(case: Case, d: dict, form: str = 'centred'):
    """(f64 reference, f32 bound) of a built case."""
    a = (d['x'], d['gamma'], d['beta'], d['eps'])
    if case.op == 'ln':
        return layernorm_ref(*a), layernorm_bound(*a, form)
    if case.op == 'gelu':
        return layernorm_gelu_ref(*a), layernorm_gelu_bound(*a)
    return rmsnorm_ref(*a), rmsnorm_bound(*a)


def case_e(case: Case, d: dict) -> float:
    if case.op == 'rms':
        return ((case.C + 1) / 2 + 8) * U
    return max_e(d['x'], d['eps'], 4.0 if case.op == 'gelu' else 2.0)


def useful(case: Case, d: dict) -> bool:
    """Condition 2 and the validity of SECOND, for the wider of the two LayerNorm forms."""
    ref, bound = reference(case, d, 'nm' if case.op == 'ln' else 'centred')
    return float(bound.max()) <= USEFUL * float(ref.abs().max()) and case_e(case, d) <= E_MAX


@functools.lru_cache(maxsize=None)
def max_ratio(case: Case) -> float:
    """The largest power of two (<= 2^14) at which the case is still `useful`; found on f64 quantities only."""
    for k in range(14, 5, -1):
        if useful(case, _build(case, 2.0**k)):
            return 2.0**k
    raise AssertionError(f'{case.name}: no offset / sigma above 32 meets condition 2')


def make_case(case: Case) -> dict:
    """The inputs of a case (f32, CPU, deterministic): x [n, C, H, W], gamma, beta (scale, offset for 'rms'), eps, the constant and the
    all-zero token (or None where the map is too small for them), and the ratio used."""
    return _build(case, max_ratio(case) if case.ratio == MAX else float(case.ratio))


SWEEP_C = (1, 3, 4, 5, 8, 9, 30, 210, 252, 255, 256, 257, 260, 380, 383, 384, 385, 388, 1024, 1028)
GEOMETRIES = ((1, 1, 1), (3, 3, 3), (1, 8, 8), (3, 7, 9), (2, 1, 130))
FORM_C = (36, 300, 400)
COND_C = (180, 320, 400)
COND_EPS = (1e-5, 1e-6)
COND_RATIO = (1.0, 30.0, MAX)
SMALL_C = (1, 3, 8, 30, 44, 210)
SMALL_GEOMETRIES = ((2, 1, 1), (2, 7, 9), (1, 16, 17))

SWEEP = [Case(f'sweep-C{c}', 'ln', c, 2, 5, 13, seed=1) for c in SWEEP_C]
GEOMETRY = [Case(f'geom-C{c}-{n}x{h}x{w}', 'ln', c, n, h, w, seed=2) for c in (20, 392) for n, h, w in GEOMETRIES]
GRID = Case('grid-C8-725x725', 'ln', 8, 1, 725, 725, seed=3)
FORMS = [Case(f'forms-C{c}', 'ln', c, 2, 5, 13, seed=4) for c in FORM_C]
CONDITIONING = [Case(f'cond-C{c}-eps{e:g}-r{r}', 'ln', c, 2, 5, 13, eps=e, ratio=r, seed=5) for c in COND_C for e in COND_EPS for r in COND_RATIO]
BRACKETS = [Case(f'bracket-C{c}', 'ln', c, 2, 5, 13, ratio=30.0, seed=6, embed=180) for c in (180, 300, 400)]
GELU = [Case(f'gelu-C{c}-{n}x{h}x{w}', 'gelu', c, n, h, w, seed=7) for c in SMALL_C for n, h, w in SMALL_GEOMETRIES]
RMS = [Case(f'rms-C{c}-{n}x{h}x{w}', 'rms', c, n, h, w, eps=1e-6, seed=8) for c in SMALL_C for n, h, w in SMALL_GEOMETRIES]
ALL_CASES = SWEEP + GEOMETRY + [GRID] + FORMS + CONDITIONING + BRACKETS + GELU + RMS
WORST = next(c for c in CONDITIONING if c.C == 400 and c.eps == 1e-6 and c.ratio == MAX)  # the worst-conditioned case
