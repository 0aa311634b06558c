"""The UniUpsample heads shared by MoSRv2 (reference ``archs/mosrv2/arch.py:91-172``) and FDAT's UniUpsampleV3 (``archs/fdat/arch.py:291-440``,
its first five modes): conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample, as one ``Head`` object a module builds in its
constructor and asks for its parameter shapes, its packed weights and its launches.

conv / pixelshuffledirect store through depth-to-space; pixelshuffle (LeakyReLU 0.01) re-lays its shuffled stores out as planes;
nearest+conv reads its x2^n stages through the convolution's nearest-upsample-on-read, and at x3 the convolution before the upsampling is
stored with every output channel repeated 9 times through depth-to-space, which IS the nearest x3 map; dysample is the shared DySample head
(engine/dysample.py) after the optional mid_dim conv + LeakyReLU 0.01.  With a 3x3 end convolution (``end_kernel=3``) the convolution runs
AFTER the sampling, at output resolution: rsa_dysample samples the features themselves, 8 channels per launch through a selection matrix, and
the convolution reads them as planes.
"""

from __future__ import annotations

import math

import torch

from . import dysample as dys
from . import lib as L
from . import ops
from .tensors import Planes

SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')
SAMPLE_MODS3 = SAMPLE_MODS + ('transpose+conv', 'lda', 'pa_up')  # UniUpsampleV3's; the last three have no layers here
GROUPS = 4  # DySample


def head_layers(upsample: str, scale: int, in_dim: int, out_dim: int, mid_dim: int):
    """UniUpsample's layers with parameters: [(index, cout, cin, k)], and the DySample sub-module's index (or None)."""
    if scale == 1 or upsample == 'conv':
        return [(0, out_dim, in_dim, 3)], None
    if upsample == 'pixelshuffledirect':
        return [(0, out_dim * scale * scale, in_dim, 3)], None
    pow2 = scale & (scale - 1) == 0
    if upsample in ('pixelshuffle', 'nearest+conv') and not pow2 and scale != 3:
        raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
    if upsample == 'pixelshuffle':
        layers, i = [(0, mid_dim, in_dim, 3)], 2
        for r in [2] * int(math.log2(scale)) if pow2 else [3]:
            layers.append((i, r * r * mid_dim, mid_dim, 3))
            i += 2
        return layers + [(i, out_dim, mid_dim, 3)], None
    if upsample == 'nearest+conv':
        layers, i = [], 0
        for _ in range(int(math.log2(scale)) if pow2 else 1):
            layers.append((i, in_dim, in_dim, 3))
            i += 3
        return layers + [(i, in_dim, in_dim, 3), (i + 2, out_dim, in_dim, 3)], None
    if upsample == 'dysample':
        if mid_dim != in_dim:
            return [(0, mid_dim, in_dim, 3)], 2
        return [], 0
    raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')


class Head:
    """One UniUpsample under the key prefix ``prefix`` (e.g. 'to_img', 'upscale'): ``layers`` [(index, cout, cin, k)] and ``dys_index`` as
    ``head_layers`` gives them.  ``version`` is what the MetaUpsample buffer records (and 3 = UniUpsampleV3's list of modes; of its last three
    the head has no layers: ``layers`` is None and the module emits them itself); ``meta_mid_dim``: the width that buffer records where it
    is not the one the layers use."""

    def __init__(self, prefix: str, upsample: str, scale: int, in_dim: int, out_dim: int, mid_dim: int, end_kernel: int = 1, version: int = 2,
                 meta_mid_dim: int | None = None) -> None:  # fmt: skip
        self.prefix, self.upsample, self.scale, self.in_dim, self.out_dim, self.mid_dim = prefix, upsample, scale, in_dim, out_dim, mid_dim
        self.end_kernel, self.version, self.meta_mid_dim = end_kernel, version, mid_dim if meta_mid_dim is None else meta_mid_dim
        self.layers, self.dys_index = (None, None) if scale != 1 and upsample in SAMPLE_MODS3[len(SAMPLE_MODS) :] else head_layers(upsample, scale, in_dim, out_dim, mid_dim)
        self.dys_dim = mid_dim if self.dys_index else in_dim  # the width DySample samples
        self.dys3 = self.dys_index is not None and end_kernel == 3

    def macs(self) -> int:
        return sum(co * ci * k * k for _, co, ci, k in self.layers)

    def shapes(self, shapes: dict, buffers: dict, whole_planes: str | None = None) -> None:
        """The MetaUpsample buffer, the parameter shapes and DySample's ``init_pos`` buffer.  ``whole_planes``: the name of a family whose
        kernels need the hidden widths to fill planes of 8 channels."""
        if whole_planes and (any(co % 8 for _, co, _, _ in self.layers[:-1]) or (self.dys_index == 2 and self.mid_dim % 8)):
            raise NotImplementedError(f"{whole_planes}: the head's hidden widths must be multiples of 8")
        index = (SAMPLE_MODS3 if self.version == 3 else SAMPLE_MODS).index(self.upsample)
        meta = [self.version, index, self.scale, self.in_dim, self.out_dim, self.meta_mid_dim, GROUPS]
        buffers[f'{self.prefix}.MetaUpsample'] = torch.tensor(meta, dtype=torch.uint8)
        for i, co, ci, k in self.layers or []:
            shapes[f'{self.prefix}.{i}.weight'] = (co, ci, k, k)
            shapes[f'{self.prefix}.{i}.bias'] = (co,)
        if self.dys_index is not None:
            d, s, c, k = f'{self.prefix}.{self.dys_index}', self.scale, self.dys_dim, self.end_kernel
            if c <= GROUPS or c % GROUPS:
                raise ValueError('Incorrect in_channels and groups values.')
            shapes[f'{d}.end_conv.weight'] = (self.out_dim, c, k, k)
            shapes[f'{d}.end_conv.bias'] = (self.out_dim,)
            shapes[f'{d}.offset.weight'] = (2 * GROUPS * s * s, c, 1, 1)
            shapes[f'{d}.offset.bias'] = (2 * GROUPS * s * s,)
            shapes[f'{d}.scope.weight'] = (2 * GROUPS * s * s, c, 1, 1)
            buffers[f'{d}.init_pos'] = dys.dysample_init_pos(s, GROUPS)

    def pack(self, W: dict, sd: dict, products, device, run: int | None = None, dys_pos: torch.Tensor | None = None) -> None:
        """Pack the layers into ``W`` as 'head0', 'head1', ... (and DySample's tensors).  ``run``, ``dys_pos``: the width DySample's features
        are stored at and the position of every channel in it, where the module lays them out (default: ``dys_dim`` wide, in order)."""
        cw = lambda w, b: ops.ConvWeights.from_oihw(w, b, products, device=device)  # noqa: E731
        for j, (i, co, ci, k) in enumerate(self.layers):
            w, b = sd[f'{self.prefix}.{i}.weight'], sd[f'{self.prefix}.{i}.bias']
            if self.upsample == 'nearest+conv' and self.scale == 3 and j == 0:
                # conv -> Upsample(3): every output channel 9 times, stored through depth-to-space (channel 9c + k -> sub-pixel k of c)
                w, b = w.repeat_interleave(9, 0), b.repeat_interleave(9, 0)
            W[f'head{j}'] = cw(w, b)
        if self.dys_index is None:
            return
        d = f'{self.prefix}.{self.dys_index}'
        end_w, end_b = sd[f'{d}.end_conv.weight'], sd[f'{d}.end_conv.bias']
        if self.dys3:
            c = self.dys_dim
            run, pos = c if run is None else run, torch.arange(c) if dys_pos is None else dys_pos
            W['dys.end3'] = cw(end_w, end_b)
            # row o of the selection matrix picks the feature the reference has at channel o: buffer channel pos[o]
            sel = torch.zeros(((c + 7) // 8 * 8, run), dtype=torch.float32, device=device)
            sel[torch.arange(c, device=device), pos.to(device)] = 1.0
            W['dys.sel'] = [sel[8 * g : 8 * g + 8].contiguous() for g in range((c + 7) // 8)]
            W['dys.zero'] = torch.zeros(8, dtype=torch.float32, device=device)
            end_w, end_b = torch.zeros((8, run), device=device), W['dys.zero']
        dys.pack(W, sd[f'{d}.offset.weight'], sd[f'{d}.offset.bias'], sd[f'{d}.scope.weight'], end_w.reshape(end_w.shape[0], -1), end_b,
                 sd[f'{d}.init_pos'], GROUPS, self.scale, products=products, device=device)  # fmt: skip

    def needs_f32_input(self, W: dict) -> bool:
        """Whether ``emit`` reads an f32 map of the head's input (DySample sampling the input features themselves)."""
        return self.dys_index == 0 and dys.needs_f32_input(W)

    def emit(self, plan, W: dict, fe: Planes, fe32, y, with_lo: bool, run: int | None = None) -> None:  # noqa: C901
        """Emit the head from the feature planes ``fe`` (``in_dim`` channels; ``fe32`` its f32 map when ``needs_f32_input``) into the output
        tensor ``y`` [n, out, s H, s W].  ``run``: the width the hidden layers run at where the module pads it (default ``mid_dim``)."""
        s, layers, n, H, Wd = self.scale, self.layers, fe.n, fe.h, fe.w
        mid = self.mid_dim if run is None else run
        if s == 1 or self.upsample in ('conv', 'pixelshuffledirect'):
            plan.conv(ops.conv_params(W['head0'], fe, H, Wd, out_nchw=y, pixel_shuffle=1 if self.upsample == 'conv' or s == 1 else s))
            return
        if self.upsample == 'dysample':
            x, x32 = fe, fe32
            if self.dys_index == 2:
                x = plan.planes(n, mid // 8, H, Wd, with_lo)
                x32 = plan.f32map(n, mid, H, Wd) if dys.needs_f32_input(W) else None
                plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.01, out=x, out_f32=x32))
            if self.dys3:
                self._emit_dys3(plan, W, x, x32, y, with_lo)
            else:
                dys.emit(plan, W, x, y, x32)
            return
        if self.upsample == 'pixelshuffle':
            t = plan.planes(n, mid // 8, H, Wd, with_lo)
            plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.01, out=t))
            hh, ww = H, Wd
            for j in range(1, len(layers) - 1):
                r = math.isqrt(layers[j][1] // self.mid_dim)
                shuffled = torch.empty((n, mid, hh * r, ww * r), dtype=torch.float32, device=plan.device)
                plan.keep.append(shuffled)
                plan.conv(ops.conv_params(W[f'head{j}'], t, hh, ww, out_nchw=shuffled, pixel_shuffle=r))
                hh, ww = hh * r, ww * r
                t = plan.planes(n, mid // 8, hh, ww, with_lo)
                plan.call(lambda src=shuffled, dst=t: ops.nchw_to_planes(src, dst))
                plan.count_launches(1)
            plan.conv(ops.conv_params(W[f'head{len(layers) - 1}'], t, hh, ww, out_nchw=y))
            return
        # nearest+conv: conv -> Upsample -> LeakyReLU(0.2) per stage (the activation commutes with the nearest upsampling)
        dim = self.in_dim
        pd = (dim + 7) // 8
        t, hh, ww = fe, H, Wd
        stages = len(layers) - 2
        upsampled = False
        if s == 3:
            shuffled = torch.empty((n, dim, 3 * H, 3 * Wd), dtype=torch.float32, device=plan.device)
            plan.keep.append(shuffled)
            plan.conv(ops.conv_params(W['head0'], fe, H, Wd, act=L.ACT_LRELU, act_param=0.2, out_nchw=shuffled, pixel_shuffle=3))
            hh, ww = 3 * H, 3 * Wd
            t = plan.planes(n, pd, hh, ww, with_lo)
            plan.call(lambda src=shuffled, dst=t: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
        else:
            for j in range(stages):
                o = plan.planes(n, pd, hh * 2 if upsampled else hh, ww * 2 if upsampled else ww, with_lo)
                if upsampled:
                    hh, ww = hh * 2, ww * 2
                plan.conv(ops.conv_params(W[f'head{j}'], t, hh, ww, upsample2x=upsampled, act=L.ACT_LRELU, act_param=0.2, out=o))
                t, upsampled = o, True
        if upsampled:
            hh, ww = hh * 2, ww * 2
        o = plan.planes(n, pd, hh, ww, with_lo)
        plan.conv(ops.conv_params(W[f'head{stages}'], t, hh, ww, upsample2x=upsampled, act=L.ACT_LRELU, act_param=0.2, out=o))
        plan.conv(ops.conv_params(W[f'head{stages + 1}'], o, hh, ww, out_nchw=y))

    def _emit_dys3(self, plan, W: dict, x: Planes, x32, y, with_lo: bool) -> None:
        """DySample with its 3x3 end convolution from the features ``x`` / ``x32``: the offsets, then the sampled FEATURES at output
        resolution (rsa_dysample, 8 channels per launch through a selection matrix) as planes, and the end convolution on them."""
        s, n, H, Wd = self.scale, x.n, x.h, x.w
        offscope = plan.f32map(n, 4 * GROUPS * s * s, H, Wd)
        plan.conv(ops.conv_params(W['dys.offscope'], x, H, Wd, out_f32=offscope))
        up = plan.planes(n, len(W['dys.sel']), s * H, s * Wd, with_lo)
        d = W['dys']
        for g, sel in enumerate(W['dys.sel']):
            t = torch.empty((n, 8, s * H, s * Wd), dtype=torch.float32, device=plan.device)
            plan.keep.append(t)
            dp = L.DySampleParams()
            dp.batch, dp.H, dp.W, dp.C, dp.groups, dp.scale, dp.out_ch = n, H, Wd, sel.shape[1], GROUPS, s, 8
            dp.x_f32, dp.offscope = x32.data_ptr(), offscope.data_ptr()
            dp.init_pos, dp.end_b, dp.end_w = d['init_pos'].data_ptr(), W['dys.zero'].data_ptr(), sel.data_ptr()
            dp.out_nchw, dp.out_dtype = t.data_ptr(), L.F32
            plan.launch('rsa_dysample', dp)
            one = Planes(up.hi[:, g : g + 1], None if up.lo is None else up.lo[:, g : g + 1])
            plan.call(lambda src=t, dst=one: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
        plan.conv(ops.conv_params(W['dys.end3'], up, s * H, s * Wd, out_nchw=y))


class OwnMetaUpsample:
    """Mixin of a module whose ``up`` is its ``Head``: as the reference's ``load_state_dict`` overrides, the module's own MetaUpsample buffer
    wins over the checkpoint's."""

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        state_dict = dict(state_dict)
        state_dict[f'{self.up.prefix}.MetaUpsample'] = self.get_buffer(f'{self.up.prefix}.MetaUpsample')
        return super().load_state_dict(state_dict, strict=strict, assign=assign)
