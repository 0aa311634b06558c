"""The fused convolution's epilogue (csrc/conv_common.h: ``epilogue`` / ``epilogue_impl``) at every dispatch boundary, against float64.

One case table drives three things:

* ``epilogue_ref`` restates the contract of ``rsa_conv_params`` (include/resselt_amd.h) in float64 torch on the CPU -- conv, bias, activation,
  ``* alpha + res1``, ``* beta + res2``, ``* out_scale + out_shift[oc]``, ``+ base``, depth-to-space, rounding -- from the operand values the
  kernel sees (planes rounded to hi + lo of their format, 8-bit lo codes decoded, base images in their own dtype).  A CPU test checks it
  against ``torch.nn`` modules (Compact's tail, ``nn.PReLU``, the RDB / RRDB residual formula).
* a CPU test builds every case's descriptor on host tensors (nothing is launched) and asserts the kernel family
  (``rsa_conv_kernel_name``) and the weight layout the case is meant to hit, so a case cannot drift to another kernel unnoticed.
* the GPU tests run every case and compare all of the output (pre-filled with NaN / 0xFF / a sentinel) with the reference.

Tolerances (no new constants).  Arithmetic term per operand mode, times max|pre-store reference|: ``TOL`` of tests/test_conv_gpu.py for three
and one bf16 products, the constants of tests/test_conv_fp16_gpu.py for one (1e-5) and three (3e-6) fp16 products.  On top of it only the
destination's rounding: half an ulp of f16 (2^-11 relative) / bf16 (2^-8 relative) for plain tensors; for planes the comparisons of those two
files (bf16 hi + lo: max(arith, 1e-5) * 1.5; fp16 hi + lo: arith + 2e-6; fp16 hi only: arith + 2^-11 * 1.01; 8-bit lo codes: the code's step,
2^-19); bf16 hi only: arith + 2^-8.  An 8-bit image ``u`` passes iff ``|u - 255 * clamp(ref, 0, 1)| <= 0.5 + 255 * arith * scale``.

Measured on an MI355X: the largest error of each case family as a fraction of its tolerance.  Where the destination keeps 8 or 11 bits the
figure is its half ulp (close to 1 by construction); the arithmetic alone is the "arithmetic only" row and the f32 / hi + lo rows.

    final store, arithmetic only (error beyond half an ulp of the dtype)   bf16x3 0.15   bf16 0.00   fp16 0.02   fp16x3 0.17
    final store into f32 / f16 / bf16, three bf16 products                  0.15 / 0.93 / 0.98
    final store, one fp16 product f32 / f16 / bf16; three: f32 / f16        0.02 / 0.94 / 0.98;  0.17 / 0.97
    final store, 8-bit image (beyond the 0.5 of the rounding)               0.05
    planes, three bf16 products: folded bf16 hi + lo / generic hi + lo      0.28 / 0.22      bf16 hi only 0.72   fp16 hi + lo 0.05   hi + lo8 0.13
    planes, one fp16 product: folded fp16 hi / hi + lo                      0.71 / 0.02      generic hi 0.73   hi + lo 0.04   hi + lo8 0.22   bf16 0.37
    planes, three fp16 products: folded fp16 hi / hi + lo                   0.73 / 0.06      generic hi 0.91   hi + lo 0.12   hi + lo8 0.54   bf16 0.37
    f32 map next to planes: bf16x3 / fp16 / fp16x3                          0.16 / 0.05 / 0.21
    conv5 from the ring (XRES) taken / refused                              0.24 / 0.23
    growth pair fused / launched one by one (fp16 hi planes)                0.76 / 0.76
"""

import ctypes as C
import functools
import math
from dataclasses import dataclass

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from test_conv_gpu import TOL

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops, tensors
from resselt_amd.engine.tensors import PF_BF16, PF_F16

gpu = pytest.mark.gpu

MODES = {'bf16x3': (3, PF_BF16), 'bf16': (1, PF_BF16), 'fp16': (1, PF_F16), 'fp16x3': (3, PF_F16)}  # operand mode -> (products, in_fmt)
# arithmetic tolerance against a float reference, relative to max|reference|: tests/test_conv_gpu.py (TOL), tests/test_conv_fp16_gpu.py
# (one fp16 product against the convolution of the rounded operands: 1e-5; three fp16 products: 3e-6)
ARITH = {'bf16x3': TOL[3], 'bf16': TOL[1], 'fp16': 1e-5, 'fp16x3': 3e-6}
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16, 'u8': torch.uint8}
HALF_ULP = {'f32': 0.0, 'f16': 2.0**-11, 'bf16': 2.0**-8}
CPU = torch.device('cpu')


# ---------------------------------------------------------------------------------------------------------------- operands as the kernel sees them
def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _q16(x):
    """bf16 hi + lo (16 significant bits), as the split planes hold a value."""
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def _h16(x):
    return x.half().float()


def _h22(x):
    """fp16 hi + lo (22 significant bits)."""
    hi = x.half().float()
    return hi + (x - hi).half().float()


def _seen(x, fmt, lo):
    """The value a kernel reads from planes of format ``fmt`` holding ``x``, with (``lo``) or without their lo halves."""
    if fmt == PF_F16:
        return _h22(x) if lo else _h16(x)
    return _q16(x) if lo else x.bfloat16().float()


def _f32(v):
    """A Python float as the descriptor's float field holds it."""
    return C.c_float(v).value


def _units(t):
    """[N, C, H, W] (C a multiple of 8) -> the plane layout [N, C / 8, H, W, 8]."""
    n, c, h, w = t.shape
    return t.reshape(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the float64 reference
def _act64(v, act, slope):
    if act == 'none':
        return v
    if act == 'gelu':
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == 'prelu':  # per-channel slopes [C]
        return torch.where(v >= 0, v, v * slope.double().view(1, -1, 1, 1))
    assert act == 'lrelu'
    return torch.where(v >= 0, v, v * _f32(slope))


def epilogue_ref(x, w, b, *, up=False, act='none', slope=0.0, res1=None, alpha=1.0, res2=None, beta=1.0, out_scale=1.0, out_shift=None, base=None,
                 base_div=0, ps=1):  # fmt: skip
    """``rsa_conv_params`` in float64: [nearest x2] -> conv (k = 1 | 3, zero padding) + bias -> activation -> ``* alpha + res1`` -> ``* beta + res2``
    -> ``* out_scale + out_shift[oc]`` -> depth-to-space by ``ps`` -> ``+ base`` pixel ``(min(Y // div, h - 1), min(X // div, w - 1))`` (``div`` =
    ``base_div``, or ``ps`` over the H x W base of ``base_div = 0``; the base is added per OUTPUT pixel, so adding it after the shuffle is the
    same sum as the header's order).  Every operand is taken as given: round them first to what the kernel reads.  Returns the value before
    it is rounded to the output's dtype."""
    x = x.double()
    if up:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    v = F.conv2d(x, w.double(), None if b is None else b.double(), padding=w.shape[-1] // 2)
    v = _act64(v, act, slope)
    if res1 is not None:
        v = v * _f32(alpha) + res1.double()
    if res2 is not None:
        v = v * _f32(beta) + res2.double()
    v = v * _f32(out_scale)
    if out_shift is not None:  # indexed by the OUTPUT channel oc = c // ps^2
        v = v + out_shift.double().repeat_interleave(ps * ps).view(1, -1, 1, 1)
    if ps > 1:
        v = F.pixel_shuffle(v, ps)
    if base is not None:
        div = base_div if base_div > 0 else ps
        ys = torch.clamp(torch.arange(v.shape[2]) // div, max=base.shape[2] - 1)
        xs = torch.clamp(torch.arange(v.shape[3]) // div, max=base.shape[3] - 1)
        v = v + base.double()[:, :, ys][:, :, :, xs]
    return v


def test_reference_against_torch_nn():
    """``epilogue_ref`` is itself checked: three tails of the reference architectures as ``torch.nn`` modules in float64."""
    torch.manual_seed(0)
    n, c, h, w, r = 2, 16, 7, 9, 2
    x, img = _rand((n, c, h, w), 1), _rand((n, 3, h, w), 2)
    # Compact's tail: conv -> PixelShuffle -> + F.interpolate(x, scale_factor, 'nearest')
    conv = nn.Conv2d(c, 3 * r * r, 3, padding=1).double()
    want = nn.PixelShuffle(r)(conv(x.double())) + F.interpolate(img.double(), scale_factor=r, mode='nearest')
    got = epilogue_ref(x, conv.weight.detach(), conv.bias.detach(), ps=r, base=img)
    assert (got - want.detach()).abs().max().item() <= 1e-12
    # ... and the base image of an UNPADDED input under a padded grid (base_div > 0): equal where the unpadded image is, clamped beyond
    small = img[:, :, : h - 1, : w - 2]
    up3 = F.interpolate(small.double(), scale_factor=r, mode='nearest')
    got = epilogue_ref(x, conv.weight.detach(), conv.bias.detach(), ps=r, base=small, base_div=r)
    plain = nn.PixelShuffle(r)(conv(x.double())).detach()
    assert (got[:, :, : up3.shape[2], : up3.shape[3]] - (plain[:, :, : up3.shape[2], : up3.shape[3]] + up3)).abs().max().item() <= 1e-12
    assert (got[:, :, -1, -1] - (plain[:, :, -1, -1] + small.double()[:, :, -1, -1])).abs().max().item() <= 1e-12  # last row / column: the clamp
    # nn.PReLU(num_parameters=C) with slopes outside [0, 1]
    prelu = nn.PReLU(num_parameters=12).double()
    with torch.no_grad():
        prelu.weight.copy_(torch.linspace(-0.5, 1.5, 12))
    want = prelu(conv(x.double()))
    got = epilogue_ref(x, conv.weight.detach(), conv.bias.detach(), act='prelu', slope=prelu.weight.detach())
    assert (got - want.detach()).abs().max().item() <= 1e-12
    # the residual dense block's and the RRDB's residual: (conv5(cat) * 0.2 + x) * 0.2 + x0, LeakyReLU on the growth convolutions
    conv5 = nn.Conv2d(c, c, 3, padding=1).double()
    x0 = _rand((n, c, h, w), 3)
    want = (conv5(x.double()) * _f32(0.2) + x.double()) * _f32(0.2) + x0.double()
    got = epilogue_ref(x, conv5.weight.detach(), conv5.bias.detach(), res1=x, alpha=0.2, res2=x0, beta=0.2)
    assert (got - want.detach()).abs().max().item() <= 1e-12
    want = nn.LeakyReLU(_f32(0.2))(conv5(x.double()))
    got = epilogue_ref(x, conv5.weight.detach(), conv5.bias.detach(), act='lrelu', slope=0.2)
    assert (got - want.detach()).abs().max().item() <= 1e-12
    want = nn.GELU()(conv5(F.interpolate(x.double(), scale_factor=2, mode='nearest'))) * _f32(0.5) + torch.tensor([0.1] * c).double().view(1, -1, 1, 1)
    got = epilogue_ref(x, conv5.weight.detach(), conv5.bias.detach(), up=True, act='gelu', out_scale=0.5, out_shift=torch.tensor([0.1] * c))
    assert (got - want.detach()).abs().max().item() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    id: str
    kernel: str  # substring of rsa_conv_kernel_name (the whole name where it has no template arguments)
    layout: int  # rsa_conv_weight_layout
    mode: str = 'bf16x3'
    cin: int = 64
    cout: int = 3
    k: int = 3
    up: bool = False
    n: int = 2
    h: int = 17  # 2 x 2 tiles of 16 x 32 pixels with one-pixel ragged edges
    w: int = 33
    ring: int | None = None  # rsa_debug_set_ring while the descriptor is built (None: the default schedule)
    act: str = 'none'  # none | lrelu | prelu | gelu
    slope: float = 0.2
    # final store (out = 'nchw')
    out: str = 'nchw'
    ps: int = 1
    dtype: str = 'f32'
    scale: float = 1.0
    shift: bool = False
    base: int | None = None  # None, 0 (same grid: H x W base), or out_base_div with a base one row and column short of covering the output
    # plane epilogue (out = 'planes' | 'f32': planes [+ f32 map] | the f32 map alone)
    out_fmt: int = PF_BF16
    out_lo: str = 'lo'  # 'lo' | 'none' | 'lo8'
    out_f32: bool = False
    res1: str | None = None  # None | 'f32' | 'hilo' | 'hi' | 'lo8' | 'self' (the first `cout` channels of the layer's own input planes)
    res2: str | None = None
    res_fmt: int = PF_BF16
    alpha: float = 0.37
    beta: float = -1.25
    folded: bool = False  # documentation: the case is meant to take a folded epilogue shape (EM 1..3) / a specialised kernel


_RING2F, _RING3F = 'rsa::conv_ring<2,0,1> (', 'rsa::conv_ring<3,0,1,HM> ('
_RING3F1, _RING3F3 = 'rsa::conv_ring<3,0,1,HM,f16,1> (', 'rsa::conv_ring<3,0,1,HM,f16,3> ('
_OUTK1, _PP, _CK, _GEMM = 'rsa::conv_kernel<..., OUTK=1> (final store)', 'rsa::conv_kernel_pp', 'rsa::conv_kernel', 'rsa::gemm_k1_kernel'

FINAL = [
    # two-stream ring, whole chunks, three bf16 products: Cout <= 32 (Cout <= 16: one live cout tile)
    Case('r2-ps1-c3-f32', _RING2F, 1, cout=3),
    Case('r2-ps1-c3-u8', _RING2F, 1, cout=3, dtype='u8', scale=0.9, shift=True),
    Case('r2-ps1-c3-f16-base0-lrelu', _RING2F, 1, cout=3, dtype='f16', base=0, act='lrelu'),
    Case('r2-ps2-c12-f16-affine-lrelu', _RING2F, 1, cout=12, ps=2, dtype='f16', scale=0.7, shift=True, act='lrelu'),  # scalar path: a ragged tile
    Case('r2-ps2-c12-f32-base0-prelu', _RING2F, 1, cout=12, ps=2, base=0, act='prelu'),
    Case('r2-ps2-c12-bf16-div2-scale', _RING2F, 1, cout=12, ps=2, dtype='bf16', base=2, scale=0.9),  # out_scale without out_shift, scalar path
    Case('r2-ps2-c24-f32', _RING2F, 1, cout=24, ps=2),  # tile 0 on the vector path, tile 1 on the scalar path
    Case('r2-ps2-c24-bf16-affine-prelu', _RING2F, 1, cout=24, ps=2, dtype='bf16', scale=1.3, shift=True, act='prelu'),
    Case('r2-ps2-c24-u8', _RING2F, 1, cout=24, ps=2, dtype='u8'),
    Case('r2-ps3-c27-f32-div3-prelu', _RING2F, 1, cout=27, ps=3, base=3, act='prelu'),  # no vector path for a factor of 3
    Case('r2-ps3-c27-f16-div2-affine', _RING2F, 1, cout=27, ps=3, dtype='f16', base=2, scale=0.8, shift=True),
    Case('r2-ps4-c16-f16-affine', _RING2F, 1, cout=16, ps=4, dtype='f16', scale=0.5, shift=True),  # a single whole tile
    Case('r2-ps4-c16-bf16-gelu', _RING2F, 1, cout=16, ps=4, dtype='bf16', act='gelu'),
    Case('r2-ps4-c16-u8', _RING2F, 1, cout=16, ps=4, dtype='u8', scale=1.1, shift=True),
    Case('r2-ps2-c12-f32-3x5', _RING2F, 1, cout=12, ps=2, h=3, w=5, shift=True),  # one tile, smaller than the halo
    Case('r2-ps2-c24-f16-1x40', _RING2F, 1, cout=24, ps=2, dtype='f16', h=1, w=40),
    # three cout tiles: Cout 33..48, whole chunks (layout 1) and half chunks (layout 2)
    Case('r3-ps4-c48-f32', _RING3F, 1, cout=48, ps=4),
    Case('r3-ps4-c48-bf16-shift-half', _RING3F, 2, cin=48, cout=48, ps=4, dtype='bf16', shift=True),
    Case('r3-ps2-c48-f32-lrelu-half', _RING3F, 2, cin=48, cout=48, ps=2, act='lrelu'),
    Case('r3-ps2-c48-bf16-scale', _RING3F, 1, cout=48, ps=2, dtype='bf16', scale=1.2),  # out_scale without out_shift, vector path
    Case('r3-ps4-c48-bf16-base0', _RING3F, 1, cout=48, ps=4, dtype='bf16', base=0),
    Case('r3-ps2-c48-f32-div2', _RING3F, 1, cout=48, ps=2, base=2),  # a base image sends whole tiles down the scalar path
    Case('r3-ps4-c48-u8-half', _RING3F, 2, cin=48, cout=48, ps=4, dtype='u8'),
    Case('r3-ps4-c48-f16-prelu', _RING3F, 1, cout=48, ps=4, dtype='f16', act='prelu'),
    Case('r3-ps2-c48-f16-gelu-3x5', _RING3F, 1, cout=48, ps=2, dtype='f16', act='gelu', h=3, w=5),
    Case('h1-ps4-c48-f16-lrelu-half', _RING3F1, 2, mode='fp16', cin=48, cout=48, ps=4, dtype='f16', act='lrelu'),
    Case('h1-ps2-c48-f32-base0-half', _RING3F1, 2, mode='fp16', cin=48, cout=48, ps=2, base=0),
    Case('h1-ps2-c48-u8-half', _RING3F1, 2, mode='fp16', cin=48, cout=48, ps=2, dtype='u8'),
    Case('h1-ps4-c48-bf16-shift', _RING3F1, 1, mode='fp16', cout=48, ps=4, dtype='bf16', shift=True),
    Case('h3-ps4-c48-f32-half', _RING3F3, 2, mode='fp16x3', cin=48, cout=48, ps=4),
    Case('h3-ps2-c48-f16-div2-prelu', _RING3F3, 1, mode='fp16x3', cout=48, ps=2, dtype='f16', base=2, act='prelu'),
    # chunk-barrier kernel, final-store instantiation
    Case('k1-ps2-c24-f32', _OUTK1, 0, k=1, cout=24, ps=2),
    Case('k1-ps3-c27-bf16-div3-prelu', _OUTK1, 0, k=1, cout=27, ps=3, dtype='bf16', base=3, act='prelu'),
    Case('k1-ps8-c192-f16', _OUTK1, 0, k=1, cout=192, ps=8, dtype='f16'),
    Case('odd-ps2-c12-f32-lrelu', _OUTK1, 0, cin=24, cout=12, ps=2, act='lrelu'),  # an odd number of input planes
    Case('odd-ps4-c48-f16-shift', _OUTK1, 0, cin=24, cout=48, ps=4, dtype='f16', shift=True),
    Case('odd-ps1-c3-u8', _OUTK1, 0, cin=24, cout=3, dtype='u8'),
    Case('pp-ps3-c27-f32-odd', _PP, 0, cin=24, cout=27, ps=3, shift=True),  # 17..32 channels in three products: the two-stage kernel's final store
    Case('p1-ps2-c24-f32', _OUTK1, 0, mode='bf16', cout=24, ps=2),  # one bf16 product
    Case('p1-ps4-c16-bf16-gelu', _OUTK1, 0, mode='bf16', cout=16, ps=4, dtype='bf16', act='gelu'),
    Case('up-ps4-c48-f32', _OUTK1, 0, up=True, cout=48, ps=4, h=18, w=34),  # fused nearest x2
    Case('up-ps2-c12-f16-base0-prelu', _OUTK1, 0, up=True, cout=12, ps=2, dtype='f16', base=0, act='prelu', h=18, w=34),
    Case('slab-ps8-c192-f32', _OUTK1, 0, cout=192, ps=8),  # three slabs of four cout tiles
    Case('slab-ps8-c192-bf16-div2-affine', _OUTK1, 0, cout=192, ps=8, dtype='bf16', base=2, scale=0.6, shift=True),
]


def _plane_carrier(mode, cout, ring, cin):
    products, fmt = MODES[mode]
    ct = (cout + 15) // 16
    if ring == 0 or cin % 16:
        return (_PP if products == 3 and ct == 2 else _CK), 0
    layout = 1 if cin % 32 == 0 else 2
    if fmt == PF_BF16:
        return {2: 'rsa::conv_ring<2,UP,0> (', 3: 'rsa::conv_ring<3,0,0,HM> (', 4: 'rsa::conv_ring<1,UP,0> ('}[ct], layout
    tag = f'f16,{products}> ('
    return {2: 'rsa::conv_ring<2,0,0,0,' + tag, 3: 'rsa::conv_ring<3,0,0,HM,' + tag, 4: 'rsa::conv_ring<1,0,0,0,' + tag}[ct], layout


_SPAN = 'rsa::conv_ring<3,0,0,HM,f16,1,XRES 3> ('
_XRES = 'rsa::conv_ring<1,0,0,0,f16,1,XRES> ('


def _plane_cases():
    """The hand-over matrix of ``epilogue()``: per operand mode, Cout (= the kernel's cout-tile template arguments) and schedule, the three folded
    shapes (EM 1: no residual; EM 2 / EM 3: one / two plane residuals with hi + lo) and, next to each, the descriptors that differ from it in ONE
    clause of the selection and must take the generic body."""
    out = []
    for mode, couts, rings in (('bf16x3', (32, 48, 64), (1, 0)), ('fp16', (32, 48, 64), (1, 0)), ('fp16x3', (32, 48, 64), (1, 0))):
        pf = MODES[mode][1]
        other = PF_F16 if pf == PF_BF16 else PF_BF16
        for cout in couts:
            cin = 48 if cout == 48 else 64  # 48: half chunks (the ring's half mode)
            for ring in rings:
                def add(tag, cout=cout, cin=cin, **kw):
                    kw.setdefault('out', 'planes')
                    kw.setdefault('out_fmt', pf)
                    kw.setdefault('res_fmt', pf)
                    kernel, layout = _plane_carrier(mode, cout, ring, cin)
                    # the one-product fp16 forms with a kernel of their own
                    span = (mode == 'fp16' and ring == 1 and cout == 48 and kw['out_fmt'] == PF_F16 and not kw.get('out_f32') and kw.get('res1') is None
                            and kw.get('res2') is None and kw.get('out_lo', 'lo') != 'lo8'
                            and (kw.get('act', 'none') == 'none' or (kw.get('act') == 'lrelu' and 0.0 <= kw.get('slope', 0.2) <= 1.0)))  # fmt: skip
                    if span:
                        kernel = _SPAN
                    out.append(Case(f'{mode}-c{cout}-ring{ring}-{tag}', kernel, layout, mode=mode, cin=cin, cout=cout, ring=ring, **kw))

                em1_lo = 'none' if pf == PF_F16 else 'lo'  # EM 1 writes hi + lo in bf16 and hi only in fp16
                for s in (0.2, 0.0, 1.0):
                    add(f'em1-slope{s}', act='lrelu', slope=s, out_lo=em1_lo, folded=True)
                    add(f'em2-slope{s}', act='lrelu', slope=s, res1='hilo', folded=True)
                    add(f'em3-slope{s}', act='lrelu', slope=s, res1='hilo', res2='hilo', folded=True)
                for s in (-0.25, 1.5):  # max(v, v * slope) is wrong here: the generic body
                    add(f'em1-slope{s}', act='lrelu', slope=s, out_lo=em1_lo)
                    add(f'em2-slope{s}', act='lrelu', slope=s, res1='hilo')
                    add(f'em3-slope{s}', act='lrelu', slope=s, res1='hilo', res2='hilo')
                add('em1-none', out_lo=em1_lo, folded=True)
                add('em3-none', res1='hilo', res2='hilo', folded=True)
                add('em1-prelu', act='prelu', out_lo=em1_lo)
                add('em2-prelu', act='prelu', res1='hilo')
                add('em3-prelu', act='prelu', res1='hilo', res2='hilo')
                add('em1-other-lo', out_lo='lo' if pf == PF_F16 else 'none')  # fp16 hi + lo / bf16 hi only: not EM 1
                add('em2-hi-only-out', res1='hilo', out_lo='none')
                add('em2-res1-hi', res1='hi')  # res1_lo == NULL with an hi + lo output
                add('em3-res2-hi', res1='hilo', res2='hi')
                add('em3-res1-hi', res1='hi', res2='hilo')
                add('res2-alone', res2='hilo')
                add('em2-res-other-fmt', res1='hilo', res_fmt=other)
                add('em3-res-other-fmt', res1='hilo', res2='hilo', res_fmt=other)
                add('em2-out-other-fmt', res1='hilo', out_fmt=other)
                add('res1-f32-res2-planes', res1='f32', res2='hilo')
                add('res1-planes-res2-f32', res1='hilo', res2='f32')
                add('em1-res1-f32', res1='f32', out_lo=em1_lo)
                add('em1-with-f32-map', out_f32=True, out_lo=em1_lo, act='lrelu')
                add('em3-with-f32-map', out_f32=True, res1='hilo', res2='hilo')
                add('f32-map-alone', out='f32', out_f32=True, res1='hilo')
                # 8-bit lo codes on ONE operand (they exist for fp16 planes only; a layer that multiplies bf16 planes may still read / write them)
                add('lo8-res1', res1='lo8', res2='hilo', res_fmt=PF_F16, out_fmt=PF_F16)
                add('lo8-res2', res1='hilo', res2='lo8', res_fmt=PF_F16, out_fmt=PF_F16)
                add('lo8-out', res1='hilo', out_lo='lo8', res_fmt=PF_F16, out_fmt=PF_F16)
                if cout != 64:  # Cout % 8 == 0 but not % 16: a half-filled last cout tile
                    c2 = 24 if cout == 32 else 40
                    add(f'em2-c{c2}', cout=c2, res1='hilo')
                    add(f'em3-c{c2}', cout=c2, res1='hilo', res2='hilo', act='lrelu')
                    add(f'em1-c{c2 - 4}-f32res', cout=c2 - 4, res1='f32', out_lo='lo')  # Cout % 8 != 0: zero-padded channels in the last plane
    # nearest x2 + 3x3, 64 -> 64 into bf16 hi + lo planes: the four-phase kernel (weight layout 3) computes max(v, v * slope); other slopes
    # fall back to the nine-tap ring schedule (layout 1).  And the fused upsampling of the two-stream shape.
    up = dict(up=True, cout=64, h=18, w=34, out='planes', act='lrelu')
    for s in (0.2, 0.0, 1.0):
        out.append(Case(f'up2-slope{s}', 'rsa::conv_ring_up2 (', 3, slope=s, folded=True, **up))
    for s in (-0.25, 1.5):
        out.append(Case(f'up2-slope{s}', 'rsa::conv_ring<1,UP,0> (', 1, slope=s, **up))
    out.append(Case('up2-with-f32-map', 'rsa::conv_ring<1,UP,0> (', 1, out_f32=True, **up))
    out.append(Case('up-c32-em1', 'rsa::conv_ring<2,UP,0> (', 1, **dict(up, cout=32), folded=True))
    out.append(Case('up-c32-em1-slope1.5', 'rsa::conv_ring<2,UP,0> (', 1, **dict(up, cout=32), slope=1.5))
    # the wide 1x1 schedule's direct epilogue (gemm_k1.hip, EPI 3: fp16 hi planes, an f32 residual) has the same max(v, v * slope) form
    for s in (0.2, 0.0, 1.0, -0.25, 1.5):
        out.append(Case(f'gemm-k1-slope{s}', _GEMM, 0, mode='fp16', k=1, cout=96, out='planes', out_fmt=PF_F16, out_lo='none', res1='f32', act='lrelu',
                        slope=s, folded=0.0 <= s <= 1.0))  # fmt: skip
    return out


PLANE = _plane_cases()
ALL_CASES = FINAL + PLANE


# ---------------------------------------------------------------------------------------------------------------- building a case
class _HostWeights(ops.ConvWeights):
    """Weights of a descriptor that is only asked for its dispatch (CPU): any non-null blob pointer will do."""

    def packed_for(self, layout):
        return self.bias


def _weights(w, b, mode, device):
    products, fmt = MODES[mode]
    if device.type == 'cpu':
        cout, cin, k, _ = w.shape
        return _HostWeights(None, ops.pad_bias(b, cout, device), cout, cin, (cin + 7) // 8, k, products, fmt=fmt)
    return ops.ConvWeights.from_oihw(w, b, products, device=device, fmt=fmt)


def _guarded(shape, dtype, fill, guard, device):
    """A tensor of ``shape`` filled with ``fill`` at the front of a larger allocation whose ``guard`` trailing elements carry the same fill:
    (tensor, guard view).  A store or a load that runs past the tensor stays inside the allocation and is seen."""
    numel = math.prod(shape)
    flat = torch.full((numel + guard,), fill, dtype=dtype, device=device)
    return flat[:numel].view(shape), flat[numel:]


def _prelu_slopes(cout, seed, device):
    """Slopes in [-0.5, 1.5] with an exact 0 and an exact 1; the padding up to 16 channels carries a sentinel no output may depend on."""
    s = _rand((cout,), seed) + 0.5
    s[0], s[cout - 1] = 0.0, 1.0
    vec = torch.full(((cout + 15) // 16 * 16,), 1e6)
    vec[:cout] = s
    return s, vec.to(device)


class Built:
    pass


def _residual(kind, r, fmt, n, planes, h, w, device):
    """One residual operand of kind f32 | hilo | hi | lo8 holding ``r``: (what conv_params takes, the values the kernel reads)."""
    if kind == 'f32':
        return tensors.nchw_to_f32map(r.to(device)), r
    if kind == 'lo8':
        hi, code = tensors.lo8_encode(r)
        pl = tensors.Planes.empty(n, planes, h, w, device, False, PF_F16).with_lo8(planes)
        pl.hi.copy_(_units(hi).to(device))
        pl.lo8.copy_(_units(code).to(device))
        return (pl, 0, 'lo8'), tensors.lo8_decode(hi, code)
    pl = tensors.nchw_to_planes(r.to(device), with_lo=kind == 'hilo', fmt=fmt)
    return (pl, 0), _seen(r, fmt, kind == 'hilo')


def build(c: Case, device):
    """Operands, buffers and the descriptor of a case.  On the CPU the tensors are host tensors and nothing may be launched: the descriptor then
    only answers rsa_conv_kernel_name / rsa_conv_weight_layout."""
    t = Built()
    products, fmt = MODES[c.mode]
    seed = 1000 + sum(map(ord, c.id))
    hin, win = (c.h // 2, c.w // 2) if c.up else (c.h, c.w)
    t.x = _rand((c.n, c.cin, hin, win), seed)
    t.w = _rand((c.cout, c.cin, c.k, c.k), seed + 1, 1.0 / (c.cin * c.k * c.k) ** 0.5)
    t.b = _rand((c.cout,), seed + 2, 0.1) + (0.5 if c.dtype == 'u8' else 0.0)
    t.xs, t.wsn = _seen(t.x, fmt, products == 3), _seen(t.w, fmt, products == 3)
    t.wts = _weights(t.w, t.b, c.mode, device)
    t.xin = tensors.nchw_to_planes(t.x.to(device), with_lo=products == 3, fmt=fmt)
    kw, t.ref_kw = {}, dict(up=c.up, act=c.act)
    if c.act == 'lrelu':
        kw.update(act=L.ACT_LRELU, act_param=c.slope)
        t.ref_kw['slope'] = c.slope
    elif c.act == 'gelu':
        kw.update(act=L.ACT_GELU)
    elif c.act == 'prelu':
        slopes, t.act_vec = _prelu_slopes(c.cout, seed + 3, device)
        kw.update(act=L.ACT_PRELU, act_vec=t.act_vec)
        t.ref_kw['slope'] = slopes
    if c.out == 'nchw':
        r = c.ps
        oc, oh, ow = c.cout // (r * r), c.h * r, c.w * r
        dt = DTYPES[c.dtype]
        shape = (c.n, oh, ow, oc) if c.dtype == 'u8' else (c.n, oc, oh, ow)
        # four output planes of guard: a store that lands past the tensor is seen, and stays inside the allocation
        t.out, t.guard = _guarded(shape, dt, 0xFF if c.dtype == 'u8' else float('nan'), 4 * oh * ow, device)
        kw.update(out_nchw=t.out, pixel_shuffle=r, out_scale=c.scale)
        t.ref_kw.update(ps=r, out_scale=c.scale)
        if c.shift:
            t.shift = _rand((oc,), seed + 4, 0.3)
            t.shift_dev = t.shift.to(device)
            kw.update(out_shift=t.shift_dev)
            t.ref_kw['out_shift'] = t.shift
        if c.base is not None:
            bh, bw = (c.h, c.w) if c.base == 0 else (-(-oh // c.base) - 1, -(-ow // c.base) - 1)  # one short: the last row / column is clamped
            base = _rand((c.n, oc, bh, bw), seed + 5).to(dt)
            t.base, _ = _guarded((c.n, oc, bh, bw), dt, 1e4, 4 * bw + 4, device)  # a read past the base image finds the sentinel
            t.base.copy_(base)
            kw.update(out_base=t.base, out_base_div=c.base)
            t.ref_kw.update(base=base, base_div=c.base)
    else:
        planes = (c.cout + 7) // 8
        for name in ('res1', 'res2'):
            kind = getattr(c, name)
            if kind is not None:
                r = _rand((c.n, c.cout, c.h, c.w), seed + (6 if name == 'res1' else 7))
                kw[name], t.ref_kw[name] = _residual(kind, r, c.res_fmt, c.n, planes, c.h, c.w, device)
        kw.update(alpha=c.alpha, beta=c.beta)
        t.ref_kw.update(alpha=c.alpha, beta=c.beta)
        if c.out == 'planes':
            # written at plane offset 1 of a wider buffer: one sentinel plane on either side
            t.planes = tensors.Planes.empty(c.n, planes + 2, c.h, c.w, device, with_lo=c.out_lo == 'lo', fmt=c.out_fmt)
            t.planes.hi.fill_(7.0)
            if t.planes.lo is not None:
                t.planes.lo.fill_(7.0)
            if c.out_lo == 'lo8':
                t.planes.with_lo8(planes + 2).lo8.fill_(0x55)
            kw.update(out=t.planes, out_plane_off=1, out_lo8=c.out_lo == 'lo8')
        if c.out_f32:
            t.f32 = tensors.empty_f32map(c.n, c.cout, c.h, c.w, device)
            t.f32.fill_(float('nan'))
            kw.update(out_f32=t.f32)
    lib = L.load()
    try:
        if c.ring is not None:
            lib.rsa_debug_set_ring(c.ring)
        t.p = ops.conv_params(t.wts, t.xin, c.h, c.w, upsample2x=c.up, **kw)
    finally:
        lib.rsa_debug_set_ring(-1)
    return t


def _assert_dispatch(c: Case, p):
    name = L.conv_kernel_name(p)
    assert (name == c.kernel) if c.kernel in (_OUTK1, _PP, _CK, _GEMM) else (c.kernel in name), (c.id, name)
    assert p.w_layout == c.layout, (c.id, p.w_layout)


@functools.lru_cache(maxsize=None)
def _ref(c: Case):
    """The float64 reference of a case (before the destination's rounding), computed once."""
    t = build(c, CPU)
    return epilogue_ref(t.xs, t.wsn, t.b, **t.ref_kw)


# ---------------------------------------------------------------------------------------------------------------- CPU: dispatch of the table
def test_case_ids_are_unique_and_reach_every_carrier():
    ids = [c.id for c in ALL_CASES]
    assert len(ids) == len(set(ids))
    final = {c.kernel for c in FINAL}
    assert {_RING2F, _RING3F, _RING3F1, _RING3F3, _OUTK1} <= final
    outk1 = [c for c in FINAL if c.kernel == _OUTK1]
    assert any(c.k == 1 for c in outk1) and any(c.cin % 16 for c in outk1) and any(c.mode == 'bf16' for c in outk1)
    assert any(c.up for c in outk1) and any(c.cout > 64 for c in outk1)
    plane = {c.kernel for c in PLANE}
    want = {_CK, _PP, 'rsa::conv_ring<2,UP,0> (', 'rsa::conv_ring<3,0,0,HM> (', 'rsa::conv_ring<1,UP,0> ('}
    for prod in (1, 3):
        want |= {f'rsa::conv_ring<2,0,0,0,f16,{prod}> (', f'rsa::conv_ring<3,0,0,HM,f16,{prod}> (', f'rsa::conv_ring<1,0,0,0,f16,{prod}> ('}
    assert want <= plane, want - plane


@pytest.mark.parametrize('c', ALL_CASES, ids=lambda c: c.id)
def test_case_dispatches_to_its_kernel(c):
    """Every case of the table, built on host tensors: the kernel family and the weight layout it names."""
    _assert_dispatch(c, build(c, CPU).p)


# ---------------------------------------------------------------------------------------------------------------- GPU: running a case
def _report(family, err, tol):
    print(f'EPI {family} {err / tol if tol > 0 else 0.0:.3f} {err:.3e} {tol:.3e}')


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error: nothing launched after it gives a verdict, so the session ends here
        pytest.exit(f'device error, no further launches: {e}', returncode=3)


def _run(t, device):
    ops.run_convs([t.p], device)
    _sync()
    assert L.ring_aborts() == 0
    L.check_status('epilogue matrix')


@gpu
@pytest.mark.parametrize('c', FINAL, ids=lambda c: c.id)
def test_final_store(device, c):
    """The final-store branch (OUTK = 1) on each of its carriers: depth-to-space on the vector and the scalar path, every output dtype, the
    output affine, base images on the same and on a coarser grid (clamped on the last row and column), PReLU next to padded slopes."""
    t = build(c, device)
    _assert_dispatch(c, t.p)
    _run(t, device)
    pre = _ref(c)
    scale = max(pre.abs().max().item(), 1e-6)
    arith = ARITH[c.mode] * scale
    got = t.out.cpu()
    if c.dtype == 'u8':
        # deterministic bound, every pixel.  The image was pre-filled with 0xFF; a second run over zeros makes an unwritten byte fail whatever
        # its reference value is
        want = 255.0 * pre.clamp(0, 1).permute(0, 2, 3, 1)
        tol = 0.5 + 255.0 * arith
        t.out.zero_()
        _run(t, device)
        assert (t.guard == 0xFF).all(), 'a store landed behind the output image'
        for g in (got, t.out.cpu()):
            err = (g.double() - want).abs()
            assert (err <= tol).all(), (err.max().item(), tol, int((err > tol).sum()))
        _report('final-u8', (err - 0.5).clamp(min=0).max().item(), 255.0 * arith)
        return
    assert torch.isnan(t.guard).all(), 'a store landed behind the output tensor'
    assert torch.isfinite(got).all(), 'unwritten output elements'
    err = (got.double() - pre).abs()
    tol = arith + HALF_ULP[c.dtype] * pre.abs()
    bad = err > tol
    assert not bad.any(), (err.max().item(), arith, int(bad.sum()))
    _report(f'final-{c.mode}-{c.dtype}', (err / tol).max().item(), 1.0)
    _report(f'final-{c.mode}-arith-only', ((err - HALF_ULP[c.dtype] * pre.abs()).clamp(min=0)).max().item(), arith)


def _dest_tol(out_fmt, out_lo):
    """Rounding of a value to planes, relative to the map's scale: the terms of the plane comparisons in tests/test_conv_gpu.py (bf16 hi + lo:
    1e-5) and tests/test_conv_fp16_gpu.py (fp16 hi + lo: 2e-6; hi only: 2^-11 * 1.01); 8-bit lo codes: their step, 2^-19; bf16 hi only: half an ulp."""
    if out_lo == 'lo8':
        return 2.0**-19
    if out_fmt == PF_BF16:
        return 1e-5 if out_lo == 'lo' else 2.0**-8
    return 2e-6 if out_lo == 'lo' else 2.0**-11 * 1.01


def _plane_tol(mode, out_fmt, out_lo):
    """Relative tolerance of a plane output against the float reference, as those two files compare planes."""
    a = ARITH[mode]
    if out_fmt == PF_BF16 and out_lo == 'lo':
        return max(a, 1e-5) * 1.5
    return a + _dest_tol(out_fmt, out_lo)


def _check_planes(c, t, pre, scale):
    planes = (c.cout + 7) // 8
    pl = t.planes
    sub = tensors.Planes(pl.hi[:, 1 : 1 + planes].contiguous(), None if pl.lo is None else pl.lo[:, 1 : 1 + planes].contiguous(),
                         None if pl.lo8 is None else pl.lo8[:, 1 : 1 + planes].contiguous())  # fmt: skip
    full = tensors.planes_to_nchw(sub, planes * 8, lo8=c.out_lo == 'lo8').cpu()
    assert torch.isfinite(full).all()
    err = (full[:, : c.cout].double() - pre).abs().max().item()
    tol = _plane_tol(c.mode, c.out_fmt, c.out_lo) * scale
    assert err <= tol, (err, tol)
    if planes * 8 > c.cout:  # channels padded up to the plane boundary are exact zeros
        assert full[:, c.cout :].abs().max().item() == 0.0
    # the planes on either side of the written range keep their sentinel
    for s in (slice(0, 1), slice(1 + planes, None)):
        assert (pl.hi[:, s].float() == 7.0).all()
        assert pl.lo is None or (pl.lo[:, s].float() == 7.0).all()
        assert pl.lo8 is None or (pl.lo8[:, s] == 0x55).all()
    return err, tol, full[:, : c.cout]


@gpu
@pytest.mark.parametrize('c', PLANE, ids=lambda c: c.id)
def test_plane_epilogue_handover(device, c):
    """Each folded epilogue shape and the neighbours one clause away from it (see ``_plane_cases``), on both schedules."""
    t = build(c, device)
    _assert_dispatch(c, t.p)
    _run(t, device)
    pre = _ref(c)
    scale = max(pre.abs().max().item(), 1e-6)
    dest = 'f32map' if c.out == 'f32' else ('bf16' if c.out_fmt == PF_BF16 else 'fp16') + {'lo': '-hi+lo', 'none': '-hi', 'lo8': '-hi+lo8'}[c.out_lo]
    fam = f'plane-{c.mode}-{"folded" if c.folded else "generic"}-{dest}'
    vals = None
    if c.out == 'planes':
        err, tol, vals = _check_planes(c, t, pre, scale)
        _report(fam, err, tol)
    if c.out_f32:
        m = tensors.f32map_to_nchw(t.f32, c.cout).cpu()
        assert torch.isfinite(m).all(), 'unwritten elements of the f32 map'
        err = (m.double() - pre).abs().max().item()
        assert err <= ARITH[c.mode] * scale, (err, ARITH[c.mode] * scale)
        _report(f'plane-{c.mode}-f32map', err, ARITH[c.mode] * scale)
        if vals is not None:  # the planes are the f32 map's values rounded to the plane format
            assert (vals.double() - m.double()).abs().max().item() <= _dest_tol(c.out_fmt, c.out_lo) * scale


# ---------------------------------------------------------------------------------------------------------------- the specialised forms
# conv5 of a dense block in one fp16 product with residual 1 = the layer's own first 64 input channels (conv_ring_xres_eligible): the slopes
# the form computes as max(v, v * slope), and the sets of 8-bit lo operands it is compiled for, each next to a descriptor it must refuse.
# (two residuals, slope or None, lo of res1 / res2 / out: 'lo' | 'lo8', taken by the XRES form)
XRES = [(two, s, 'lo', 'lo', 'lo', s is None or 0.0 <= s <= 1.0) for two in (False, True) for s in (None, 0.2, 0.0, 1.0, -0.25, 1.5)] + [
    (False, None, 'lo8', 'lo', 'lo', True),
    (False, None, 'lo8', 'lo', 'lo8', True),
    (False, None, 'lo', 'lo', 'lo8', False),
    (True, None, 'lo8', 'lo8', 'lo', True),
    (True, 0.2, 'lo8', 'lo8', 'lo8', True),
    (True, None, 'lo8', 'lo', 'lo', False),
    (True, None, 'lo', 'lo8', 'lo8', False),
    (True, None, 'lo8', 'lo', 'lo8', False),
    (True, 1.5, 'lo8', 'lo8', 'lo8', False),
]
_XRES_IDS = [f'{"two" if a[0] else "one"}-slope{a[1]}-{a[2]}-{a[3]}-{a[4]}' for a in XRES]


def _stream64(pl, v, lo, device):
    """Store the 64-channel map ``v`` into the first 8 planes of the fp16 workspace ``pl`` (hi + fp16 lo, or hi + 8-bit codes); returns the
    values a kernel reads back."""
    if lo == 'lo8':
        hi, code = tensors.lo8_encode(v)
        pl.lo8.copy_(_units(code).to(device))
        seen = tensors.lo8_decode(hi, code)
    else:
        hi = v.half()
        lo16 = (v - hi.float()).half()
        pl.lo.copy_(_units(lo16).to(device))
        seen = hi.float() + lo16.float()
    pl.hi[:, :8] = _units(hi).to(device)
    return seen


def build_xres(device, two, slope, r1, r2, olo):
    t = Built()
    n, h, w, cin = 2, 17, 33, 96
    t.x = _rand((n, cin, h, w), 71, 1.5)
    t.w = _rand((64, cin, 3, 3), 72, 1.0 / (cin * 9) ** 0.5)
    t.b = _rand((64,), 73, 0.1)
    t.wts = _weights(t.w, t.b, 'fp16', device)

    def workspace():
        pl = tensors.Planes.empty(n, cin // 8, h, w, device, True, PF_F16, lo_planes=8).with_lo8(8)
        pl.hi.zero_()
        pl.lo.zero_()
        pl.lo8.zero_()
        return pl

    t.ws = workspace()
    res1 = _stream64(t.ws, t.x[:, :64], r1, device)
    t.ws.hi[:, 8:] = _units(t.x[:, 64:].half()).to(device)
    kw = dict(res1=(t.ws, 0, 'lo8') if r1 == 'lo8' else (t.ws, 0), alpha=0.2)
    t.ref_kw = dict(res1=res1, alpha=0.2)
    if two:
        t.r0 = workspace()  # another workspace: both residuals share their strides
        res2 = _stream64(t.r0, _rand((n, 64, h, w), 74), r2, device)
        kw.update(res2=(t.r0, 0, 'lo8') if r2 == 'lo8' else (t.r0, 0), beta=0.2)
        t.ref_kw.update(res2=res2, beta=0.2)
    if slope is not None:
        kw.update(act=L.ACT_LRELU, act_param=slope)
        t.ref_kw.update(act='lrelu', slope=slope)
    t.out = tensors.Planes.empty(n, 8, h, w, device, True, PF_F16).with_lo8(8)
    t.out.hi.fill_(float('nan'))
    t.p = ops.conv_params(t.wts, t.ws, h, w, cin_planes=cin // 8, out=t.out, out_lo8=olo == 'lo8', **kw)
    return t


def _assert_xres(p, taken):
    name = L.conv_kernel_name(p)
    assert p.w_layout == 1 and ((_XRES in name) if taken else ('rsa::conv_ring<1,0,0,0,f16,1> (' in name)), name


@pytest.mark.parametrize('two,slope,r1,r2,olo,taken', XRES, ids=_XRES_IDS)
def test_xres_dispatch(two, slope, r1, r2, olo, taken):
    _assert_xres(build_xres(CPU, two, slope, r1, r2, olo).p, taken)


@gpu
@pytest.mark.parametrize('two,slope,r1,r2,olo,taken', XRES, ids=_XRES_IDS)
def test_xres_conv5_and_its_fallback(device, two, slope, r1, r2, olo, taken):
    t = build_xres(device, two, slope, r1, r2, olo)
    _assert_xres(t.p, taken)
    _run(t, device)
    pre = epilogue_ref(_h16(t.x), _h16(t.w), t.b, **t.ref_kw)  # the multiply reads hi halves only
    scale = pre.abs().max().item()
    got = tensors.planes_to_nchw(tensors.Planes(t.out.hi, None if olo == 'lo8' else t.out.lo, t.out.lo8), 64, lo8=olo == 'lo8').cpu()
    assert torch.isfinite(got).all()
    err, tol = (got.double() - pre).abs().max().item(), _plane_tol('fp16', PF_F16, olo) * scale
    assert err <= tol, (err, tol)
    _report(f'xres-{"taken" if taken else "fallback"}', err, tol)


# two consecutive growth convolutions of a dense block (conv_pair_eligible -> conv_ring_em1_eligible): slopes of (a, b), fused by the list launch
PAIR = [(0.2, 0.2, True), (None, 1.0, True), (0.0, 0.2, True), (0.2, 1.5, False), (-0.25, 0.2, False)]


def build_pair(device, sa, sb):
    t = Built()
    n, h, w, cin = 2, 17, 33, 64
    t.x = _rand((n, cin, h, w), 81)
    t.w = [_rand((32, cin, 3, 3), 82, 1.0 / (cin * 9) ** 0.5), _rand((32, cin + 32, 3, 3), 83, 1.0 / ((cin + 32) * 9) ** 0.5)]
    t.b = [_rand((32,), 84, 0.1), _rand((32,), 85, 0.1)]
    t.wts = [_weights(t.w[i], t.b[i], 'fp16', device) for i in range(2)]
    t.ws = tensors.Planes.empty(n, 24, h, w, device, True, PF_F16, lo_planes=8)
    t.ws.hi.fill_(7.0)
    t.ws.lo.fill_(7.0)
    t.ws.hi[:, :8] = _units(t.x.half()).to(device)
    act = lambda s: dict(act=L.ACT_NONE) if s is None else dict(act=L.ACT_LRELU, act_param=s)  # noqa: E731
    t.p = [ops.conv_params(t.wts[0], t.ws, h, w, cin_planes=8, out=t.ws, out_plane_off=8, **act(sa)),
           ops.conv_params(t.wts[1], t.ws, h, w, cin_planes=12, out=t.ws, out_plane_off=12, **act(sb))]  # fmt: skip
    return t


def _assert_pair(t, fusable):
    try:
        L.set_pair_fusion(1)
        assert all(p.w_layout == 1 and 'rsa::conv_ring<2,0,0,0,f16,1> (' in L.conv_kernel_name(p) for p in t.p)
        assert L.conv_pair_fusable(*t.p) == fusable
    finally:
        L.set_pair_fusion(-1)


@pytest.mark.parametrize('sa,sb,fusable', PAIR)
def test_pair_dispatch(sa, sb, fusable):
    _assert_pair(build_pair(CPU, sa, sb), fusable)


@gpu
@pytest.mark.parametrize('sa,sb,fusable', PAIR)
def test_pair_and_its_fallback(device, sa, sb, fusable):
    """A pair whose slopes the fused kernel computes, and pairs it must leave to the layer-wise kernels: the list launch is right either way."""
    t = build_pair(device, sa, sb)
    _assert_pair(t, fusable)
    try:
        L.set_pair_fusion(1)
        ops.run_convs(t.p, device)
        _sync()
    finally:
        L.set_pair_fusion(-1)
    assert L.ring_aborts() == 0
    L.check_status('pair')
    cat = _h16(t.x)
    for i, s in enumerate((sa, sb)):
        kw = {} if s is None else dict(act='lrelu', slope=s)
        pre = epilogue_ref(cat, _h16(t.w[i]), t.b[i], **kw)
        got = tensors.planes_to_nchw(tensors.Planes(t.ws.hi[:, 8 + 4 * i : 12 + 4 * i].contiguous(), None), 32).cpu()
        scale = pre.abs().max().item()
        err, tol = (got.double() - pre).abs().max().item(), _plane_tol('fp16', PF_F16, 'none') * scale
        assert err <= tol, (i, err, tol)
        _report(f'pair-{"fused" if fusable else "fallback"}', err, tol)
        cat = torch.cat((cat, got), 1)  # b reads a's ROUNDED output
    assert (t.ws.hi[:, 16:] == 7.0).all() and (t.ws.lo == 7.0).all()


# channel sums in the epilogue (conv_pool_eligible): compiled for max(v, v * slope) only; anything else is refused, nothing launched
POOL = [('bf16x3', 0.2, True), ('fp16', 1.0, True), ('bf16x3', 1.5, False), ('fp16', -0.25, False)]


def build_pool(device, mode, slope):
    t = build(Case('pool', '', 1, mode=mode, cout=64, out='planes', out_fmt=MODES[mode][1], act='lrelu', slope=slope), device)
    t.slots = ops.conv_pool_slots(t.p)
    return t


@pytest.mark.parametrize('mode,slope,taken', POOL)
def test_pool_dispatch(mode, slope, taken):
    assert (build_pool(CPU, mode, slope).slots is not None) == taken


@gpu
@pytest.mark.parametrize('mode,slope,taken', [c for c in POOL if not c[2]])
def test_pool_sums_refuses_other_slopes(device, mode, slope, taken):
    t = build_pool(device, mode, slope)
    assert t.slots is None
    sums = torch.zeros((2, 64, 64), dtype=torch.float32, device=device)
    t.p.pool_sums = sums.data_ptr()
    assert L.load().rsa_conv2d(C.byref(t.p), C.c_void_p(ops.current_stream_ptr(device))) == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(sums.abs().max()) == 0.0 and (t.planes.hi.float() == 7.0).all()  # nothing was launched
    L.check_status('pool')
