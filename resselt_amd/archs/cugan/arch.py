"""Real-CUGAN on the MI355X engine (reference module: ``resselt/archs/cugan/arch.py``): UpCunet2x / 3x / 4x / 2x_fast, ``alpha = 1``.

Geometry.  Each U-Net stage lives on one grid (a plane buffer of fixed size); every tensor of the reference is a window (origin + size)
of a grid.  A valid 3x3 convolution runs as the zero-padded rsa_conv2d on the whole grid and shrinks the window by one pixel per side
(border pixels are computed and ignored); ``F.pad(x, (-k,) * 4)`` shrinks a window without touching memory.  rsa_conv_s2 writes its
output at (window origin // 2) of the half-size grid and pairs pixels from the window's own origin (UNet2's second down convolution
reads a window at an odd coordinate); rsa_deconv writes the up path straight into the window of the skip tensor it is added to, the
skip add and the LeakyReLU in its epilogue.  The plan is a host-side list of ``Layer`` records (``cugan_layers``) that the GPU plan
and the CPU replay of tests/test_cugan_loader.py both execute.

SE.  The gate of an SEBlock feeds the next down / up convolution and a later skip add; rsa_region_se applies it once, in place, to the
window.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import torch

from ...engine import cugan as CG
from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Fp16Range, Plan, check_fp16_range
from ...engine.cugan import Win
from ...engine.paramtree import build_param_tree

VARIANTS = ('2x', '3x', '4x', '2x_fast')
# reflect pad of the input (arch.py:303-305, 346-348, 390-392, 427-430) and the multiple the padded size is rounded to
_PAD = {'2x': (18, 2), '3x': (14, 4), '4x': (19, 2), '2x_fast': (38, 2)}
_SCALE = {'2x': 2, '3x': 3, '4x': 4, '2x_fast': 2}
PRO_SCALE, PRO_SHIFT = 0.7, 0.15


@dataclass
class Layer:
    """One launch of the plan.  ``op``: 'conv3' (3x3, zero pad 1, on the whole grid), 'conv_s2', 'deconv', 'se' (in place).
    ``win_in`` / ``win_out`` are windows of the ``src`` / ``dst`` grids; a residual is read at ``win_out`` of ``res``."""

    op: str
    key: str
    src: str
    dst: str
    win_in: Win
    win_out: Win
    lrelu: bool = False
    res: str | None = None
    ksize: int = 3
    stride: int = 1
    pad: int = 0


@dataclass
class Buf:
    grid: str
    channels: int
    planes: bool = True  # split planes (read by a later convolution)
    f32: bool = False  # f32 map [N][C/4][H][W][4]


@dataclass
class Geometry:
    grids: dict = field(default_factory=dict)  # name -> (H, W)
    bufs: dict = field(default_factory=dict)  # name -> Buf
    layers: list = field(default_factory=list)
    pad_top: int = 0
    pad_left: int = 0
    unshuffle: int = 1
    out_map: str = ''
    out_origin: tuple = (0, 0)
    pixel_shuffle: int = 1
    out_hw: tuple = (0, 0)
    base_div: int = 0  # > 0: the nearest-upsampled input is added (4x, 2x_fast)


def _need(win: Win, what: str) -> Win:
    if win.h < 1 or win.w < 1:
        raise ValueError(f'CUGAN: the input is too small ({what} would be empty)')
    return win


def _same(a: int, b: int, what: str) -> None:
    if a != b:
        raise ValueError(f'CUGAN: the input size gives mismatched U-Net maps at {what} ({a} vs {b}); the reference fails there too')


def _unet_conv(g: Geometry, key: str, src: str, grid: str, win: Win, cmid: int, cout: int, se: bool, out: str) -> Win:
    mid = out + '_mid'
    g.bufs[mid] = Buf(grid, cmid)
    g.bufs[out] = Buf(grid, cout)
    w1 = _need(win.shrink(1), key)
    g.layers.append(Layer('conv3', f'{key}.conv.0', src, mid, win, w1, lrelu=True))
    w2 = _need(w1.shrink(1), key)
    g.layers.append(Layer('conv3', f'{key}.conv.2', mid, out, w1, w2, lrelu=True))
    if se:
        g.layers.append(Layer('se', f'{key}.seblock', out, out, w2, w2))
    return w2


def _down(g: Geometry, key: str, src: str, win: Win, grid: str, out: str, cout: int) -> Win:
    g.bufs[out] = Buf(grid, cout)
    wo = _need(Win(win.y0 // 2, win.x0 // 2, win.h // 2, win.w // 2), key)
    g.layers.append(Layer('conv_s2', key, src, out, win, wo, lrelu=True, ksize=2, stride=2))
    return wo


def _up(g: Geometry, key: str, src: str, win: Win, skip: str, skip_win: Win, out: str, cout: int) -> Win:
    g.bufs[out] = Buf(g.bufs[skip].grid, cout)
    _same(2 * win.h, skip_win.h, key)
    _same(2 * win.w, skip_win.w, key)
    g.layers.append(Layer('deconv', key, src, out, win, skip_win, lrelu=True, res=skip, ksize=2, stride=2))
    return skip_win


def cugan_layers(variant: str, in_ch: int, out_ch: int, h0: int, w0: int) -> Geometry:
    """The launch records of one forward for an h0 x w0 input; ``ValueError`` where the reference fails (reflect pad >= size, U-Net maps
    that do not match)."""
    if variant not in VARIANTS:
        raise ValueError(f'unknown CUGAN variant {variant!r}')
    s = _SCALE[variant]
    pad, mult = _PAD[variant]
    ph, pw = -(-h0 // mult) * mult, -(-w0 // mult) * mult
    for lo, hi, n in ((pad, pad + ph - h0, h0), (pad, pad + pw - w0, w0)):
        if lo >= n or hi >= n:
            raise ValueError(f'CUGAN {variant}: a {h0}x{w0} input is too small (reflect padding {max(lo, hi)} needs a size above it)')
    g = Geometry()
    g.pad_top = g.pad_left = pad
    r = 2 if variant == '2x_fast' else 1
    if (ph + 2 * pad) % r or (pw + 2 * pad) % r:
        raise ValueError('CUGAN: the padded input is not divisible by the unshuffle factor')
    H0, W0 = (ph + 2 * pad) // r, (pw + 2 * pad) // r
    g.unshuffle = r
    fast4 = variant in ('4x', '2x_fast')
    c_in = in_ch * r * r
    c1 = 64 if fast4 else out_ch  # unet1 output channels
    # ---- UNet1 (UNet1x3 for 3x)
    g.grids['g0'] = (H0, W0)
    g.grids['g1'] = (H0 // 2, W0 // 2)
    g.bufs['x'] = Buf('g0', c_in)
    w = Win(0, 0, H0, W0)
    a = _unet_conv(g, 'unet1.conv1', 'x', 'g0', w, 32, 64, False, 'u1_x1')
    d = _down(g, 'unet1.conv1_down', 'u1_x1', a, 'g1', 'u1_x2', 64)
    e = _unet_conv(g, 'unet1.conv2', 'u1_x2', 'g1', d, 128, 64, True, 'u1_x2b')
    sk = _up(g, 'unet1.conv2_up', 'u1_x2b', e, 'u1_x1', a.shrink(4), 'u1_x2c', 64)
    g.bufs['u1_x3'] = Buf('g0', 64)
    w3 = _need(sk.shrink(1), 'unet1.conv3')
    g.layers.append(Layer('conv3', 'unet1.conv3', 'u1_x2c', 'u1_x3', sk, w3, lrelu=True))
    kb, sb, pb = (5, 3, 2) if variant == '3x' else (4, 2, 3)
    hz, wz = CG.deconv_out(w3.h, kb, sb, pb), CG.deconv_out(w3.w, kb, sb, pb)
    g.grids['g2'] = (hz, wz)
    g.grids['g3'] = (hz // 2, wz // 2)
    g.grids['g4'] = (hz // 4, wz // 4)
    g.bufs['z'] = Buf('g2', c1, planes=True, f32=True)
    wz_ = Win(0, 0, hz, wz)
    g.layers.append(Layer('deconv', 'unet1.conv_bottom', 'u1_x3', 'z', w3, wz_, ksize=kb, stride=sb, pad=pb))
    # ---- UNet2
    b = _unet_conv(g, 'unet2.conv1', 'z', 'g2', wz_, 32, 64, False, 'u2_x1')
    d1 = _down(g, 'unet2.conv1_down', 'u2_x1', b, 'g3', 'u2_x2', 64)
    e2 = _unet_conv(g, 'unet2.conv2', 'u2_x2', 'g3', d1, 64, 128, True, 'u2_x2b')
    d2 = _down(g, 'unet2.conv2_down', 'u2_x2b', e2, 'g4', 'u2_x3', 128)
    e3 = _unet_conv(g, 'unet2.conv3', 'u2_x3', 'g4', d2, 256, 128, True, 'u2_x3b')
    sk3 = _up(g, 'unet2.conv3_up', 'u2_x3b', e3, 'u2_x2b', e2.shrink(4), 'u2_x3c', 128)
    e4 = _unet_conv(g, 'unet2.conv4', 'u2_x3c', 'g3', sk3, 64, 64, True, 'u2_x4')
    sk4 = _up(g, 'unet2.conv4_up', 'u2_x4', e4, 'u2_x1', b.shrink(16), 'u2_x4c', 64)
    g.bufs['u2_x5'] = Buf('g2', 64)
    w5 = _need(sk4.shrink(1), 'unet2.conv5')
    g.layers.append(Layer('conv3', 'unet2.conv5', 'u2_x4c', 'u2_x5', sk4, w5, lrelu=True))
    wsum = _need(w5.shrink(1), 'unet2.conv_bottom')
    _same(wsum.h, hz - 40, 'the final add')
    # x0 + F.pad(x, -20): the unet1 output map is the residual of unet2's last convolution
    g.bufs['sum'] = Buf('g2', c1, planes=fast4, f32=not fast4)
    g.layers.append(Layer('conv3', 'unet2.conv_bottom', 'u2_x5', 'sum', w5, wsum, res='z'))
    if fast4:
        g.bufs['final'] = Buf('g2', 12, planes=False, f32=True)
        wf = _need(wsum.shrink(1), 'conv_final')
        g.layers.append(Layer('conv3', 'conv_final', 'sum', 'final', wsum, wf))
        crop = _need(wf.shrink(1), 'the final crop')
        g.out_map, g.pixel_shuffle, g.base_div = 'final', 2, s
        g.out_origin = (crop.y0, crop.x0)
        if 2 * crop.h < h0 * s or 2 * crop.w < w0 * s:
            raise ValueError('CUGAN: the output window is smaller than the image')
    else:
        g.out_map, g.pixel_shuffle = 'sum', 1
        g.out_origin = (wsum.y0, wsum.x0)
        if wsum.h < h0 * s or wsum.w < w0 * s:
            raise ValueError('CUGAN: the output window is smaller than the image')
    g.out_hw = (h0 * s, w0 * s)
    return g


def param_shapes(variant: str, in_ch: int, out_ch: int) -> dict:
    """Parameter shapes of the reference modules, in their registration order."""
    fast4 = variant in ('4x', '2x_fast')
    u1_in = 12 if variant == '2x_fast' else in_ch
    u1_out = 64 if fast4 else out_ch
    u2_in, u2_out = (64, 64) if fast4 else (in_ch, out_ch)
    sh: dict = {}

    def conv(name, co, ci, k):
        sh[f'{name}.weight'] = (co, ci, k, k)
        sh[f'{name}.bias'] = (co,)

    def tconv(name, ci, co, k):
        sh[f'{name}.weight'] = (ci, co, k, k)
        sh[f'{name}.bias'] = (co,)

    def unet_conv(name, ci, cm, co, se):
        conv(f'{name}.conv.0', cm, ci, 3)
        conv(f'{name}.conv.2', co, cm, 3)
        if se:
            conv(f'{name}.seblock.conv1', co // 8, co, 1)
            conv(f'{name}.seblock.conv2', co, co // 8, 1)

    unet_conv('unet1.conv1', u1_in, 32, 64, False)
    conv('unet1.conv1_down', 64, 64, 2)
    unet_conv('unet1.conv2', 64, 128, 64, True)
    tconv('unet1.conv2_up', 64, 64, 2)
    conv('unet1.conv3', 64, 64, 3)
    tconv('unet1.conv_bottom', 64, u1_out, 5 if variant == '3x' else 4)
    unet_conv('unet2.conv1', u2_in, 32, 64, False)
    conv('unet2.conv1_down', 64, 64, 2)
    unet_conv('unet2.conv2', 64, 64, 128, True)
    conv('unet2.conv2_down', 128, 128, 2)
    unet_conv('unet2.conv3', 128, 256, 128, True)
    tconv('unet2.conv3_up', 128, 128, 2)
    unet_conv('unet2.conv4', 128, 64, 64, True)
    tconv('unet2.conv4_up', 64, 64, 2)
    conv('unet2.conv5', 64, 64, 3)
    conv('unet2.conv_bottom', u2_out, 64, 3)
    if fast4:
        conv('conv_final', 12, 64, 3)
    return sh


class _CUGANBase(EngineModule):
    variant = '2x'
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'fp16')
    supports_u8 = True
    # the SE blocks average over the WHOLE image: output computed tile by tile differs from the whole-image output (tiling.py warns)
    global_statistics = True
    hyperparameters: dict = {}

    def __init__(self, *, in_channels: int = 3, out_channels: int = 3, pro: bool = False):
        super().__init__()
        if in_channels != 3 or out_channels != 3:
            raise NotImplementedError(f'CUGAN: only 3 input and output channels are built (got {in_channels} -> {out_channels})')
        self.in_ch, self.out_ch = in_channels, out_channels
        self.upscale = _SCALE[self.variant]
        buffers = {'pro': torch.zeros(1)} if pro else {}
        build_param_tree(self, param_shapes(self.variant, in_channels, out_channels), buffers)

    @property
    def is_pro(self) -> bool:
        return getattr(self, 'pro', None) is not None

    def geometry(self, h0: int, w0: int) -> Geometry:
        return cugan_layers(self.variant, self.in_ch, self.out_ch, h0, w0)

    def macs_per_input_pixel(self, h0: int = 1080, w0: int = 1920) -> float:
        """MACs of the reference layers per input pixel at h0 x w0 (valid windows only)."""
        g = self.geometry(h0, w0)
        sd = {k: tuple(v.shape) for k, v in self.state_dict().items()}
        total = 0
        for ly in g.layers:
            w = sd.get(f'{ly.key}.weight')
            if ly.op == 'conv3':
                total += ly.win_out.h * ly.win_out.w * w[0] * w[1] * 9
            elif ly.op == 'conv_s2':
                total += ly.win_out.h * ly.win_out.w * w[0] * w[1] * 4
            elif ly.op == 'deconv':
                total += ly.win_in.h * ly.win_in.w * w[0] * w[1] * ly.ksize**2
        return total / (h0 * w0)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        fmt = products.fmt
        W: dict = {}
        for ly in cugan_layers(self.variant, self.in_ch, self.out_ch, 64, 64).layers:  # (every size has the same layers)
            if ly.key in W:
                continue
            if ly.op == 'conv3':
                W[ly.key] = ops.ConvWeights.from_oihw(sd[f'{ly.key}.weight'], sd[f'{ly.key}.bias'], products, device=device)
            elif ly.op in ('conv_s2', 'deconv'):
                W[ly.key] = CG.ResampleWeights.make(sd[f'{ly.key}.weight'], sd[f'{ly.key}.bias'], ly.stride, ly.pad, ly.op == 'deconv', products, fmt, device)
            else:
                k = ly.key
                W[k] = CG.SEWeights.make(sd[f'{k}.conv1.weight'], sd[f'{k}.conv1.bias'], sd[f'{k}.conv2.weight'], sd[f'{k}.conv2.bias'], device)
        if fmt == ops.PF_F16:
            check_fp16_range(W.values())
            if max((w.raw_absmax for w in W.values() if isinstance(w, CG.ResampleWeights)), default=0.0) > 6.0e4:
                raise Fp16Range('a transposed / strided convolution weight exceeds the fp16 range (|w| > 6e4)')
        return W

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        g = self.geometry(h0, w0)
        with_lo = products == 3
        dev = plan.device
        planes, maps = {}, {}
        for name, b in g.bufs.items():
            gh, gw = g.grids[b.grid]
            if b.planes:
                planes[name] = plan.planes(n, (b.channels + 7) // 8, gh, gw, with_lo)
                planes[name].hi.zero_()  # border pixels outside the windows stay finite and deterministic
                if planes[name].lo is not None:
                    planes[name].lo.zero_()
            if b.f32:
                maps[name] = plan.f32map(n, b.channels, gh, gw)
                maps[name].zero_()
        pro = self.is_pro
        in_scale, in_shift = (PRO_SCALE, PRO_SHIFT) if pro else (1.0, 0.0)

        def set_input(x):
            p = CG.input_params(x, x_shape, planes['x'], g.pad_top, g.pad_left, g.unshuffle, in_scale, in_shift)
            CG.run('rsa_cugan_input', p, device=dev)

        plan.count_launches(1)  # rsa_cugan_input, launched by set_input
        for ly in g.layers:
            if ly.op == 'conv3':
                gh, gw = g.grids[g.bufs[ly.dst].grid]
                kw = dict(act=L.ACT_LRELU, act_param=0.1) if ly.lrelu else {}
                if ly.res is not None:
                    kw['res1'] = maps[ly.res]
                out = planes.get(ly.dst) if g.bufs[ly.dst].planes else None
                plan.conv(ops.conv_params(W[ly.key], planes[ly.src], gh, gw, out=out, out_f32=maps.get(ly.dst), **kw))
            elif ly.op in ('conv_s2', 'deconv'):
                tr = ly.op == 'deconv'
                p = CG.resample_params(W[ly.key], planes[ly.src], ly.win_in, out=planes.get(ly.dst), out_f32=maps.get(ly.dst), out_y0=ly.win_out.y0,
                                       out_x0=ly.win_out.x0, res=planes.get(ly.res) if ly.res else None, res_y0=ly.win_out.y0,
                                       res_x0=ly.win_out.x0, lrelu=ly.lrelu)  # fmt: skip
                flop, nbytes = CG.resample_flop_bytes(p, tr)
                name = 'rsa_deconv' if tr else 'rsa_conv_s2'
                plan.launch(name, p, 1, meta=dict(kernel=name, layer=ly.key, flop=flop, bytes=nbytes))
                plan.keep.append(p)
            else:
                x = planes[ly.src]
                ws = CG.region_se_workspace(n, ly.win_in.h, x.planes, dev)
                gate = torch.empty((n, 8 * x.planes), dtype=torch.float32, device=dev)
                plan.keep += [ws, gate]
                p = CG.region_se_params(W[ly.key], x, ly.win_in, ws, gate)
                nbytes = n * ly.win_in.h * ly.win_in.w * x.planes * 16 * (2 if x.lo is not None else 1) * 3  # read, read + write
                plan.launch('rsa_region_se', p, 3, meta=dict(kernel='rsa_region_se', layer=ly.key, flop=0, bytes=nbytes))
                plan.keep.append(p)

        oh, ow = g.out_hw
        is_u8 = dtype == torch.uint8
        y = plan.output((n, oh, ow, self.out_ch) if is_u8 else (n, self.out_ch, oh, ow), dtype)
        base = plan.input_ref((n, h0, w0, c) if is_u8 else x_shape, dtype) if g.base_div else None
        bscale, bshift = (PRO_SCALE, PRO_SHIFT) if pro else (1.0, 0.0)
        oshift, odiv = (PRO_SHIFT, PRO_SCALE) if pro else (0.0, 1.0)
        p = CG.output_params(maps[g.out_map], self.out_ch, g.out_origin[0], g.out_origin[1], g.pixel_shuffle, y, (oh, ow), base=base,
                             base_hw=(h0, w0), base_div=max(g.base_div, 1), base_scale=bscale, base_shift=bshift, out_shift=oshift, out_div=odiv)  # fmt: skip
        plan.launch('rsa_cugan_output', p)
        return set_input


class UpCunet2x(_CUGANBase):  # the reference's class names, recorded in the fixtures' metadata
    """UpCunet2x (arch.py:274-318): UNet1 with a k4 s2 p3 transposed tail, UNet2, reflect pad 18."""

    variant = '2x'


class UpCunet3x(_CUGANBase):
    """UpCunet3x (arch.py:321-361): UNet1x3 with a k5 s3 p2 transposed tail, reflect pad 14 (multiple of 4)."""

    variant = '3x'


class UpCunet4x(_CUGANBase):
    """UpCunet4x (arch.py:364-413): 64-channel U-Nets, conv_final + PixelShuffle(2) + nearest x4 of the input, reflect pad 19."""

    variant = '4x'


class UpCunet2x_fast(_CUGANBase):  # noqa: N801
    """UpCunet2x_fast (arch.py:416-444): reflect pad 38 + pixel_unshuffle(2), 64-channel U-Nets, conv_final + PixelShuffle(2) + nearest x2."""

    variant = '2x_fast'

    def __init__(self, *, in_channels: int = 3, out_channels: int = 3):
        super().__init__(in_channels=in_channels, out_channels=out_channels, pro=False)
