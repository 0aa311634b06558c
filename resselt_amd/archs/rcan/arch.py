"""RCAN (residual channel attention network) on the MI355X engine.

Reference module: ``resselt/archs/rcan/arch.py`` (CALayer :148-164, RCAB :168-196, ResidualGroup :200-232, RCAN :236-332).  The parameter
names, shapes and order are the reference's; the forward pass is this launch list:

  * ``x * rgb_range`` and the ``sub_mean`` 1x1 convolution are ONE pointwise 3 -> 3 step on the input (``rsa_rcan_input``) with the
    checkpoint's own weights -- not folded into the zero-padded head convolution, whose border taps would then miss the bias;
  * ``unshuffle_mod``: reflect padding to a multiple of the factor and PixelUnshuffle happen in the layout kernel, the output is cropped;
  * an RCAB is two convolutions (ReLU in the first one's epilogue), the second of which also leaves per-channel partial sums of its f32
    output (``rsa_conv_params.pool_sums``), and ``rsa_rcab_tail``: the gate ``sigmoid(W2 . relu(W1 . mean + b1) + b2)`` from those sums and
    ONE pass ``x + gate * y`` that writes the planes the next convolution reads.  ``res_scale`` is ignored there, as in the reference (:194);
  * the group residual and the body residual are convolution epilogues on plane residuals;
  * the Upsampler's PixelShuffle is the store of its convolution, and ``add_mean`` with the final ``/ rgb_range`` is folded (in f64) into the
    last convolution's weights, bias and ``out_scale``.

Activations are in 0..255 units when the checkpoint has the mean shifts (``norm``), as in the reference.

Deviation: the reference's ``x *= self.rgb_range`` multiplies the CALLER's tensor in place (:323) whenever no padding copied it first.
This module never writes its input.

``rcan_fused = False`` (debug / A-B hook, read when a plan is built) runs the composed path: ``rsa_channel_gate`` re-reads the second
convolution's planes for the mean, then the same apply pass.  Shapes the pooling epilogue is not compiled for take that path too.
"""

from __future__ import annotations

import math

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import ParamShapes, build_param_tree

_MAX_HIDDEN = 128  # rsa_rcab_tail / rsa_channel_gate


class RCAN(EngineModule):
    hyperparameters = {}
    supports_u8 = True
    # 'auto' stays on three bf16 products: no one-product policy has been measured against the oracle at depth (tests/test_rcan_gpu.py pins
    # 'bf16' and 'fp16' on shallow fixtures only)
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')

    def __init__(self, *, scale: int = 4, n_resgroups: int = 10, n_resblocks: int = 20, n_feats: int = 64, n_colors: int = 3, rgb_range: int = 255,
                 norm: bool = True, kernel_size: int = 3, reduction: int = 16, res_scale: float = 1, act_mode: str = 'relu',
                 unshuffle_mod: bool = False) -> None:  # fmt: skip
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError(f'the RCAN engine runs 3x3 convolutions, got kernel_size {kernel_size}')
        if n_feats % 8:
            raise NotImplementedError('n_feats must be a multiple of 8')
        if act_mode != 'relu':
            raise NotImplementedError("the RCAN loader only builds act_mode = 'relu' models")
        hidden = n_feats // reduction
        if not 1 <= hidden <= _MAX_HIDDEN:
            raise NotImplementedError(f'n_feats // reduction must be in 1..{_MAX_HIDDEN} (the gate kernel), got {hidden}')
        self.scale = scale
        unshuffle_mod = bool(unshuffle_mod) and scale <= 2
        self.downscale_factor = 4 // scale if unshuffle_mod else 1
        self.net_scale = 4 if unshuffle_mod else scale
        if self.net_scale != 3 and (self.net_scale < 1 or self.net_scale & (self.net_scale - 1)):
            raise NotImplementedError(f'scale {self.net_scale}: the Upsampler builds 2^n and 3 only')  # as the reference's Upsampler (:143)
        self.n_resgroups, self.n_resblocks, self.n_feats, self.n_colors, self.reduction = n_resgroups, n_resblocks, n_feats, n_colors, reduction
        self.norm, self.res_scale, self.unshuffle_mod = bool(norm), res_scale, unshuffle_mod
        self.rgb_range = rgb_range if norm else 1  # (:262-270)
        self.rcan_fused: bool = True
        s = ParamShapes()
        if norm:
            s.conv('sub_mean', 3, 3, 1)  # MeanShift is nn.Conv2d(3, 3, 1) whatever n_colors is
            s.conv('add_mean', 3, 3, 1)
        df = self.downscale_factor
        self._head = 'head.1' if unshuffle_mod else 'head.0'
        s.conv(self._head, n_feats, n_colors * df * df, 3)
        for g in range(n_resgroups):
            for b in range(n_resblocks):
                p = f'body.{g}.body.{b}.body'
                s.conv(f'{p}.0', n_feats, n_feats, 3)
                s.conv(f'{p}.2', n_feats, n_feats, 3)
                s.conv(f'{p}.3.conv_du.0', hidden, n_feats, 1)
                s.conv(f'{p}.3.conv_du.2', n_feats, hidden, 1)
            s.conv(f'body.{g}.body.{n_resblocks}', n_feats, n_feats, 3)
        s.conv(f'body.{n_resgroups}', n_feats, n_feats, 3)
        self._up = []  # (layer, PixelShuffle factor)
        if self.net_scale == 3:
            self._up.append(('tail.0.0', 3))
        else:
            self._up += [(f'tail.0.{2 * i}', 2) for i in range(int(math.log2(self.net_scale)))]
        for name, r in self._up:
            s.conv(name, r * r * n_feats, n_feats, 3)
        s.conv('tail.1', n_colors, n_feats, 3)
        build_param_tree(self, s)

    def macs_per_input_pixel(self) -> int:
        """Algorithmic multiply-accumulates of the convolutions per pixel of the caller's image (the channel attention's two 1x1 layers act
        on one pooled vector per image and are not counted)."""
        f, df = self.n_feats, self.downscale_factor
        total = 9 * self.n_colors * df * df * f
        total += self.n_resgroups * (self.n_resblocks * 2 + 1) * 9 * f * f + 9 * f * f
        res = 1
        for _, r in self._up:
            total += 9 * f * r * r * f * res
            res *= r * r
        total += 9 * f * self.n_colors * res
        return total // (df * df)

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        W: dict = {}
        for name in sd:
            if name.endswith('.weight') and sd[name].shape[-1] == 3:
                base = name[: -len('.weight')]
                if base != 'tail.1':
                    W[base] = ops.ConvWeights.from_oihw(sd[name], sd[f'{base}.bias'], products, device=device)
            elif name.endswith('conv_du.0.weight'):
                p = name[: -len('.conv_du.0.weight')]
                W[f'{p}.ca'] = tuple(t.contiguous() for t in (sd[f'{p}.conv_du.0.weight'].flatten(1), sd[f'{p}.conv_du.0.bias'],
                                                               sd[f'{p}.conv_du.2.weight'].flatten(1), sd[f'{p}.conv_du.2.bias']))  # fmt: skip
        w, b = sd['tail.1.weight'].double(), sd['tail.1.bias'].double()
        if self.norm:
            # add_mean (a 1x1 convolution) behind tail.1 is one linear map of its output channels: folded in f64; `/ rgb_range` is out_scale
            a, ab = sd['add_mean.weight'].double().flatten(1), sd['add_mean.bias'].double()
            w, b = torch.einsum('oc,cikl->oikl', a, w), a @ b + ab
            W['sub_mean'] = (sd['sub_mean.weight'].flatten(1).contiguous(), sd['sub_mean.bias'].contiguous())
        W['tail.1'] = ops.ConvWeights.from_oihw(w.float(), b.float(), products, device=device)
        check_fp16_range(W.values())
        return W

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h_in, w_in = x_shape
        if c != self.n_colors:
            raise RuntimeError(f'model expects {self.n_colors} input channels, got {c}')
        if self.norm and c != 3:
            raise RuntimeError('the mean shifts are 3 -> 3 convolutions: a model with them takes 3 channels (arch.py:48)')
        df, nf = self.downscale_factor, self.n_feats
        pad_h, pad_w = (df - h_in % df) % df, (df - w_in % df) % df
        if pad_h >= h_in or pad_w >= w_in:
            raise RuntimeError(f'input {h_in}x{w_in} is too small to reflect-pad to a multiple of {df}')
        h, w = (h_in + pad_h) // df, (w_in + pad_w) // df
        with_lo = products == 3
        pf = nf // 8
        dev = plan.device
        lib = L.load()
        u8 = dtype == torch.uint8

        x_pl = plan.planes(n, (c * df * df + 7) // 8, h, w, with_lo)
        if self.norm:
            shifted = torch.empty((n, c, h_in, w_in), dtype=torch.float32, device=dev)
            plan.keep.append(shifted)
            sw, sb = W['sub_mean']

            def set_input(x):
                ops.call('rsa_rcan_input', dev, x=x, dtype=ops.rsa_dtype(x.dtype), batch=n, C=c, H=h_in, W=w_in, scale=float(self.rgb_range), weight=sw, bias=sb,
                         out=shifted)  # fmt: skip
                ops.nchw_to_planes(shifted, x_pl, unshuffle=df)  # check_img_size's reflect padding commutes with the pointwise step
        else:

            def set_input(x):
                ops.nchw_to_planes(x, x_pl, unshuffle=df)

        head_pl = plan.planes(n, pf, h, w, with_lo)
        group_pl = [plan.planes(n, pf, h, w, with_lo) for _ in range(min(2, self.n_resgroups))]
        r_pl, t_pl, y_pl = (plan.planes(n, pf, h, w, with_lo) for _ in range(3))
        relu = dict(act=L.ACT_LRELU, act_param=0.0)
        plan.conv(ops.conv_params(W[self._head], x_pl, h, w, out=head_pl))

        # the pooling epilogue is compiled for some shapes only; what it is not compiled for runs the composed path
        probe = ops.conv_params(W['body.0.body.0.body.2'], t_pl, h, w, out=y_pl) if self.n_resgroups and self.n_resblocks else None
        slots = ops.conv_pool_slots(probe) if probe is not None and self.rcan_fused else None
        fused = slots is not None
        self.rcan_fused_active = fused  # what the last built plan does (tests and tools read it)
        gate = torch.empty((n, nf), dtype=torch.float32, device=dev)
        plan.keep.append(gate)
        if fused:
            sums = torch.empty((n, slots, (nf + 15) // 16 * 16), dtype=torch.float32, device=dev)
            plan.keep.append(sums)
        elif probe is not None:
            ws_gate = torch.empty((max(int(lib.rsa_channel_gate_workspace_bytes(n, h, w, pf)), 16) // 4,), dtype=torch.float32, device=dev)
            plan.keep.append(ws_gate)
        px = n * h * w
        tail_meta = dict(name='rsa_rcab_tail', flop=2 * px * nf, bytes=px * pf * 16 * 3 * (2 if with_lo else 1))

        def rcab(p: str, x, out):
            plan.conv(ops.conv_params(W[f'{p}.0'], x, h, w, out=t_pl, **relu))
            plan.conv(ops.conv_params(W[f'{p}.2'], t_pl, h, w, out=y_pl, pool_sums=sums if fused else None))
            w1, b1, w2, b2 = W[f'{p}.3.ca']
            if not fused:
                gp = L.ChannelGateParams()
                gp.batch, gp.H, gp.W, gp.planes, gp.hidden, gp.relu = n, h, w, pf, w1.shape[0], 1
                y_pl.bind(gp, 'in')
                gp.w1, gp.b1, gp.w2, gp.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
                gp.workspace, gp.gate, gp.fmt = ws_gate.data_ptr(), gate.data_ptr(), y_pl.fmt
                plan.launch('rsa_channel_gate', gp, kernels=2)
            plan.launch('rsa_rcab_tail', dict(pool_sums=sums if fused else None, slots=slots if fused else 0, w1=w1, b1=b1, w2=w2, b2=b2, hidden=w1.shape[0],
                                              gate=gate, y=y_pl, x=x, out=out, batch=n, H=h, W=w, C=nf, fmt=y_pl.fmt),
                        kernels=2 if fused else 1, meta=tail_meta)  # fmt: skip

        cur = head_pl
        for g in range(self.n_resgroups):
            gin, x = cur, cur
            for b in range(self.n_resblocks):
                rcab(f'body.{g}.body.{b}.body', x, r_pl)  # from the second block on in place: every thread reads its unit of x before it writes it
                x = r_pl
            cur = group_pl[g & 1]
            plan.conv(ops.conv_params(W[f'body.{g}.body.{self.n_resblocks}'], x, h, w, res1=(gin, 0), alpha=1.0, out=cur))
        plan.conv(ops.conv_params(W[f'body.{self.n_resgroups}'], cur, h, w, res1=(head_pl, 0), alpha=1.0, out=r_pl))

        # tail: [conv -> PixelShuffle] per Upsampler stage into planes, then the last convolution into the output tensor
        cur, hh, ww = r_pl, h, w
        for name, r in self._up:
            shuffled = torch.empty((n, nf, hh * r, ww * r), dtype=torch.float32, device=dev)
            plan.keep.append(shuffled)
            plan.conv(ops.conv_params(W[name], cur, hh, ww, out_nchw=shuffled, pixel_shuffle=r))
            hh, ww = hh * r, ww * r
            nxt = plan.planes(n, pf, hh, ww, with_lo)
            plan.call(lambda src=shuffled, dst=nxt: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
            cur = nxt
        crop = (h_in * self.scale, w_in * self.scale) if (pad_h or pad_w) else None
        y = plan.output((n, hh, ww, c) if u8 else (n, c, hh, ww), dtype, crop)
        plan.conv(ops.conv_params(W['tail.1'], cur, hh, ww, out_nchw=y, out_scale=1.0 / self.rgb_range))
        return set_input
