"""OmniSR on the MI355X engine -- drop-in for ``resselt/archs/omni/arch.py:907-974`` in eval mode.

The input is zero-padded at the bottom / right to multiples of ``window_size``; every map below is that padded Hp x Wp map and the output is
cropped to h * s x w * s.  The residual stream is an f32 map; LayerNorms write split planes; every 1x1 / Linear layer is a k1 launch of the
convolution kernels whose residual epilogue adds into the stream.  One OSA block (:802-864), with n = LayerNorm over channels:

  MBConv     x += W3 (g * h) + b3,  h = GELU(dw3x3(GELU(W1 x + b1)) + bd),  g = sigmoid(Wb SiLU(Wa mean(h)))
             (k1 -> rsa_dwconv3x3 -> rsa_channel_gate relu = 3 -> rsa_omni_gate_scale -> k1 with the residual)
  attention  x += to_out(attn(to_qkv(n(x))))  on block, then grid windows: rsa_omni_window_attention (MFMA; eps 1e-5 LayerNorm)
  channel    x += project_out(A v),  qkv = dw3x3(W n(x)):  rsa_dwconv3x3 + rsa_omni_channel_attention, window then grid token sets
  FFN        x += project_out(GELU(dw(x1)) * dw(x2)),  [x1, x2] = project_in(n(x)):  rsa_gelu_gate_dwconv (eps 1e-6 LayerNorm2d)

in the order MBConv, block attention, FFN, window channel attention, FFN, grid attention, FFN, grid channel attention, FFN.  An OSAG is
``block_num`` blocks, a 1x1 convolution with the group input as residual, then ESA (:18-46): conv1 (k1 into an f32 map), conv2 (3x3 / stride
2) and conv3 on rsa_esa_conv3x3, the 7/3 max-pool on rsa_esa_maxpool, and rsa_esa_apply for conv_f + bilinear + conv4 + sigmoid + x * m.
Heads: 4 heads of C/4 channels each own ceil(C/32) whole planes (qkv rows and the output projection's columns are permuted at pack time).
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.transformer import LayerPacker, regroup_proj, regroup_qkv

HEADS = 4
MAX_HEAD_DIM = 32  # rsa_omni_window_attention / rsa_omni_channel_attention
MAX_ESA = 32  # rsa_esa_apply
ATTN_LN_EPS, CONV_LN_EPS = 1e-5, 1e-6
MIN_PADDED_SIDE = 15  # conv2 (3x3 / 2, no padding) then max_pool2d(7, 3) need at least one output


def esa_channels(c: int) -> int:
    return max(c // 4, 16)


def omnisr_param_shapes(in_ch: int, out_ch: int, c: int, res_num: int, block_num: int, ws: int, pe: bool, up_scale: int, bias: bool) -> ParamShapes:
    """Names and shapes of the reference module's state_dict, in its registration order."""
    s = ParamShapes()

    def conv(name, co, ci, k, b=True):
        s[f'{name}.weight'] = (co, ci, k, k)
        if b:
            s[f'{name}.bias'] = (co,)

    hid = int(c * 0.25)
    f = esa_channels(c)
    for g in range(res_num):
        for j in range(block_num):
            b = f'residual_layer.{g}.residual_layer.{j}.layer'
            conv(f'{b}.0.fn.0', c, c, 1)
            s[f'{b}.0.fn.2.weight'] = (c, 1, 3, 3)
            s[f'{b}.0.fn.2.bias'] = (c,)
            s[f'{b}.0.fn.4.gate.1.weight'] = (hid, c)
            s[f'{b}.0.fn.4.gate.3.weight'] = (c, hid)
            conv(f'{b}.0.fn.5', c, c, 1)
            for i in (2, 4, 5, 6, 8, 10, 11, 12):
                s.norm(f'{b}.{i}.norm', c)
                if i in (2, 8):  # block / grid attention
                    s[f'{b}.{i}.fn.to_qkv.weight'] = (3 * c, c)
                    s[f'{b}.{i}.fn.to_out.0.weight'] = (c, c)
                    if pe:
                        s[f'{b}.{i}.fn.rel_pos_bias.weight'] = ((2 * ws - 1) ** 2, HEADS)
                elif i in (5, 11):  # window / grid channel attention
                    s[f'{b}.{i}.fn.temperature'] = (HEADS, 1, 1)
                    s[f'{b}.{i}.fn.qkv.weight'] = (3 * c, c, 1, 1)
                    s[f'{b}.{i}.fn.qkv_dwconv.weight'] = (3 * c, 1, 3, 3)
                    s[f'{b}.{i}.fn.project_out.weight'] = (c, c, 1, 1)
                else:  # gated FFN
                    s[f'{b}.{i}.fn.project_in.weight'] = (2 * c, c, 1, 1)
                    s[f'{b}.{i}.fn.dwconv.weight'] = (2 * c, 1, 3, 3)
                    s[f'{b}.{i}.fn.project_out.weight'] = (c, c, 1, 1)
        conv(f'residual_layer.{g}.residual_layer.{block_num}', c, c, 1, bias)
        e = f'residual_layer.{g}.esa'
        conv(f'{e}.conv1', f, c, 1)
        conv(f'{e}.conv_f', f, f, 1)
        conv(f'{e}.conv2', f, f, 3)
        conv(f'{e}.conv3', f, f, 3)
        conv(f'{e}.conv4', c, f, 1)
    conv('input', c, in_ch, 3, bias)
    conv('output', c, c, 3, bias)
    conv('up.0', out_ch * up_scale * up_scale, c, 3, bias)
    return s


def _pad_rows(w: torch.Tensor, rows: int) -> torch.Tensor:
    out = torch.zeros((rows,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)
    out[: w.shape[0]] = w
    return out.contiguous()


class OmniSR(EngineModule):
    hyperparameters = {}
    precisions = ('bf16x3', 'bf16')

    def __init__(self, *, num_in_ch: int = 3, num_out_ch: int = 3, num_feat: int = 64, block_num: int = 1, pe: bool = True, window_size: int = 8,
                 res_num: int = 1, up_scale: int = 4, bias: bool = True) -> None:  # fmt: skip
        super().__init__()
        c, ws = num_feat, window_size
        if c % HEADS or c // HEADS > MAX_HEAD_DIM:
            raise NotImplementedError(f'OmniSR engine: num_feat {c} must be a multiple of {HEADS} with head_dim = num_feat / 4 <= {MAX_HEAD_DIM}')
        if not 2 <= ws <= 8:
            raise NotImplementedError(f'OmniSR engine: window_size {ws} must be 2..8 (rsa_omni_window_attention holds a window of <= 64 tokens)')
        if esa_channels(c) > MAX_ESA:
            raise NotImplementedError(f'OmniSR engine: ESA width {esa_channels(c)} > {MAX_ESA} (rsa_esa_apply)')
        if block_num < 1 or res_num < 1:
            raise NotImplementedError('OmniSR engine: res_num and block_num must be >= 1')
        self.in_ch, self.out_ch, self.dim, self.block_num, self.pe, self.ws = num_in_ch, num_out_ch, c, block_num, pe, ws
        self.res_num, self.scale, self.bias = res_num, up_scale, bias
        self.hd = c // HEADS
        self.hp = (self.hd + 7) // 8  # planes per head
        self.se_hidden = int(c * 0.25)
        self.f = esa_channels(c)
        build_param_tree(self, omnisr_param_shapes(num_in_ch, num_out_ch, c, res_num, block_num, ws, pe, up_scale, bias))

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        c, hp, pad = self.dim, self.hp, self.hp * 8
        cp = (c + 7) // 8
        pk = LayerPacker(sd, device, products, lambda name: (int(products), products.fmt))
        W, conv, lin, ln = pk.W, pk.conv, pk.lin, pk.ln
        zeros = lambda k: torch.zeros(k, dtype=torch.float32, device=device)  # noqa: E731

        def halves(w, rows_each):  # [2C, ...] -> x1 rows at 0, x2 rows at cp * 8
            out = torch.zeros((2 * rows_each,) + tuple(w.shape[1:]), dtype=torch.float32, device=device)
            out[:c] = w[:c]
            out[rows_each : rows_each + c] = w[c:]
            return out

        def head_rows(w):  # [3C, ...] -> [3 * heads * pad, ...] (which, head, d)
            t = torch.zeros((3, HEADS, pad) + tuple(w.shape[1:]), dtype=torch.float32, device=device)
            t[:, :, : self.hd] = w.reshape((3, HEADS, self.hd) + tuple(w.shape[1:]))
            return t.reshape((3 * HEADS * pad,) + tuple(w.shape[1:]))

        conv('input')
        conv('output')
        conv('up.0')
        for g in range(self.res_num):
            for j in range(self.block_num):
                b = f'residual_layer.{g}.residual_layer.{j}.layer'
                conv(f'{b}.0.fn.0')
                W[f'{b}.0.fn.2'] = (_pad_rows(sd[f'{b}.0.fn.2.weight'].reshape(c, 9), cp * 8), _pad_rows(sd[f'{b}.0.fn.2.bias'], cp * 8))
                w1 = torch.zeros((self.se_hidden, cp * 8), dtype=torch.float32, device=device)
                w1[:, :c] = sd[f'{b}.0.fn.4.gate.1.weight']
                W[f'{b}.0.fn.4'] = (w1, zeros(self.se_hidden), _pad_rows(sd[f'{b}.0.fn.4.gate.3.weight'], cp * 8), zeros(cp * 8))
                conv(f'{b}.0.fn.5')
                for i in (2, 8):
                    ln(f'{b}.{i}.norm')
                    wq, _ = regroup_qkv(sd[f'{b}.{i}.fn.to_qkv.weight'], None, HEADS, pad=pad, scale_q=True)
                    lin(f'{b}.{i}.fn.to_qkv', wq, None)
                    lin(f'{b}.{i}.fn.to_out.0', regroup_proj(sd[f'{b}.{i}.fn.to_out.0.weight'], HEADS, pad=pad), None, cin_planes=HEADS * hp)
                    if self.pe:
                        W[f'{b}.{i}.fn.rel_pos_bias'] = sd[f'{b}.{i}.fn.rel_pos_bias.weight'].contiguous()
                for i in (4, 6, 10, 12):
                    ln(f'{b}.{i}.norm')
                    lin(f'{b}.{i}.fn.project_in', halves(sd[f'{b}.{i}.fn.project_in.weight'].reshape(2 * c, c), cp * 8), None)
                    W[f'{b}.{i}.fn.dwconv'] = halves(sd[f'{b}.{i}.fn.dwconv.weight'].reshape(2 * c, 9), cp * 8).contiguous()
                    lin(f'{b}.{i}.fn.project_out', sd[f'{b}.{i}.fn.project_out.weight'].reshape(c, c), None)
                for i in (5, 11):
                    ln(f'{b}.{i}.norm')
                    W[f'{b}.{i}.fn.temperature'] = sd[f'{b}.{i}.fn.temperature'].reshape(-1).contiguous()
                    lin(f'{b}.{i}.fn.qkv', head_rows(sd[f'{b}.{i}.fn.qkv.weight'].reshape(3 * c, c)), None)
                    W[f'{b}.{i}.fn.qkv_dwconv'] = (head_rows(sd[f'{b}.{i}.fn.qkv_dwconv.weight'].reshape(3 * c, 9)).contiguous(), zeros(3 * HEADS * pad))
                    lin(f'{b}.{i}.fn.project_out', regroup_proj(sd[f'{b}.{i}.fn.project_out.weight'].reshape(c, c), HEADS, pad=pad), None,
                        cin_planes=HEADS * hp)  # fmt: skip
            conv(f'residual_layer.{g}.residual_layer.{self.block_num}')
            e = f'residual_layer.{g}.esa'
            conv(f'{e}.conv1')
            f = self.f
            W[f'{e}.conv2'] = (sd[f'{e}.conv2.weight'].contiguous(), sd[f'{e}.conv2.bias'].contiguous())
            W[f'{e}.conv3'] = (sd[f'{e}.conv3.weight'].contiguous(), sd[f'{e}.conv3.bias'].contiguous())
            W[f'{e}.apply'] = (sd[f'{e}.conv_f.weight'].reshape(f, f).contiguous(), sd[f'{e}.conv_f.bias'].contiguous(),
                               sd[f'{e}.conv4.weight'].reshape(c, f).contiguous(), sd[f'{e}.conv4.bias'].contiguous())  # fmt: skip
        return W

    def macs_per_input_pixel(self) -> int:
        """Algorithmic MACs per padded LR pixel: convolutions, Linear layers, both attention kinds, depthwise convolutions, the head."""
        c, ntok, hd, f = self.dim, self.ws * self.ws, self.hd, self.f
        mb = 2 * c * c + 9 * c
        attn = 4 * c * c + 2 * ntok * c
        chan = 4 * c * c + 27 * c + 2 * hd * c
        ffn = 3 * c * c + 18 * c
        blk = mb + 2 * attn + 2 * chan + 4 * ffn
        esa = c * f + f * f + c * f + (9 * f * f) // 4
        macs = self.res_num * (self.block_num * blk + c * c + esa)
        return macs + 9 * self.in_ch * c + 9 * c * c + 9 * c * self.out_ch * self.scale * self.scale

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, cin, h0, w0 = x_shape
        if cin != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {cin}')
        ws, c, s = self.ws, self.dim, self.scale
        H, Wd = h0 + (ws - h0 % ws) % ws, w0 + (ws - w0 % ws) % ws
        if H < MIN_PADDED_SIDE or Wd < MIN_PADDED_SIDE:
            # the reference fails in F.max_pool2d of ESA (output size 0) with a RuntimeError
            raise RuntimeError(f'OmniSR: the input {h0}x{w0} pads to {H}x{Wd}; ESA needs a padded side of at least {MIN_PADDED_SIDE}')
        with_lo = products == 3
        prod, fmt = int(products), products.fmt
        cp, hp = (c + 7) // 8, self.hp
        ap = HEADS * hp  # attention planes
        dev = plan.device
        lib = L.load()

        x_pl = plan.planes(n, (cin + 7) // 8, H, Wd, with_lo)
        xpad = None
        if (H, Wd) != (h0, w0):
            xpad = torch.zeros((n, cin, H, Wd), dtype=dtype, device=dev)
            plan.keep.append(xpad)

        def set_input(x):
            if xpad is None:
                ops.nchw_to_planes(x, x_pl)
            else:  # pad_to_multiple(mode='constant'): the border of xpad stays zero
                xpad[:, :, :h0, :w0].copy_(x)
                ops.nchw_to_planes(xpad, x_pl)

        first = plan.f32map(n, c, H, Wd)
        pool = [plan.f32map(n, c, H, Wd) for _ in range(3)]
        s_pl = plan.planes(n, cp, H, Wd, with_lo)  # the stream as planes (MBConv's input, the ESA / output convolutions' input)
        a_pl = plan.planes(n, cp, H, Wd, with_lo)  # LayerNorm outputs
        t_pl = plan.planes(n, cp, H, Wd, with_lo)
        h_pl = plan.planes(n, cp, H, Wd, with_lo)
        qkv_pl = plan.planes(n, 3 * ap, H, Wd, with_lo)
        qkv2_pl = plan.planes(n, 3 * ap, H, Wd, with_lo)
        att_pl = plan.planes(n, ap, H, Wd, with_lo)
        ffn_pl = plan.planes(n, 2 * cp, H, Wd, with_lo)
        mid_pl = plan.planes(n, cp, H, Wd, with_lo)
        gate = torch.empty((n, cp * 8), dtype=torch.float32, device=dev)
        ws_gate = torch.empty((max(int(lib.rsa_channel_gate_workspace_bytes(n, H, Wd, cp)), 16) // 4,), dtype=torch.float32, device=dev)
        ws_ca = max(int(lib.rsa_omni_channel_attn_workspace_bytes(n, H, Wd, ws, HEADS, self.hd, g)) for g in (0, 1))
        ws_attn = torch.empty((max(ws_ca, 16) // 4,), dtype=torch.float32, device=dev)
        f = self.f
        H2, W2 = (H - 3) // 2 + 1, (Wd - 3) // 2 + 1
        Hc, Wc = (H2 - 7) // 3 + 1, (W2 - 7) // 3 + 1
        c1f = plan.f32map(n, f, H, Wd)
        c2f = plan.f32map(n, f, H2, W2)
        pmf = plan.f32map(n, f, Hc, Wc)
        c3f = plan.f32map(n, f, Hc, Wc)
        plan.keep += [gate, ws_gate, ws_attn]

        def norm(name, x, eps):
            g_, b_ = W[name]
            lp = L.LayerNormParams()
            lp.batch, lp.H, lp.W, lp.C, lp.eps = n, H, Wd, c, eps
            lp.x_f32, lp.gamma, lp.beta = x.data_ptr(), g_.data_ptr(), b_.data_ptr()
            a_pl.bind(lp, 'out')
            lp.out_fmt = fmt
            plan.launch('rsa_layernorm', lp)

        def dwconv(weights, src, planes, out, act):
            dp = L.DwConvParams()
            dp.batch, dp.H, dp.W, dp.planes, dp.act, dp.fmt = n, H, Wd, planes, act, fmt
            src.bind(dp, 'in')
            dp.weight, dp.bias = weights[0].data_ptr(), weights[1].data_ptr()
            out.bind(dp, 'out')
            plan.launch('rsa_dwconv3x3', dp)

        def attn_params(src, grid):
            p = L.OmniAttnParams()
            p.batch, p.H, p.W, p.ws, p.heads, p.head_dim, p.grid, p.fmt = n, H, Wd, ws, HEADS, self.hd, grid, fmt
            src.bind(p, 'qkv')
            att_pl.bind(p, 'out')
            return p

        def mbconv(b, x, out):
            plan.conv(ops.conv_params(W[f'{b}.0.fn.0'], s_pl, H, Wd, act=L.ACT_GELU, out=t_pl))
            dwconv(W[f'{b}.0.fn.2'], t_pl, cp, h_pl, L.ACT_GELU)
            w1, b1, w2, b2 = W[f'{b}.0.fn.4']
            gp = L.ChannelGateParams()
            gp.batch, gp.H, gp.W, gp.planes, gp.hidden, gp.relu, gp.fmt = n, H, Wd, cp, self.se_hidden, 3, fmt
            h_pl.bind(gp, 'in')
            gp.w1, gp.b1, gp.w2, gp.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
            gp.workspace, gp.gate = ws_gate.data_ptr(), gate.data_ptr()
            plan.launch('rsa_channel_gate', gp, kernels=2)
            plan.launch('rsa_omni_gate_scale', dict(in_hi=h_pl.hi_ptr(), in_lo=h_pl.lo_ptr(), plane_stride=h_pl.plane_stride, batch_stride=h_pl.batch_stride,
                                                    batch=n, H=H, W=Wd, planes=cp, gate=gate, fmt=fmt, out_hi=h_pl.hi_ptr(), out_lo=h_pl.lo_ptr()))  # fmt: skip
            plan.conv(ops.conv_params(W[f'{b}.0.fn.5'], h_pl, H, Wd, res1=x, alpha=1.0, out_f32=out))

        def window_attention(b, i, x, out, grid):
            norm(f'{b}.{i}.norm', x, ATTN_LN_EPS)
            plan.conv(ops.conv_params(W[f'{b}.{i}.fn.to_qkv'], a_pl, H, Wd, out=qkv_pl))
            p = attn_params(qkv_pl, grid)
            if self.pe:
                p.bias_table = W[f'{b}.{i}.fn.rel_pos_bias'].data_ptr()
            plan.launch('rsa_omni_window_attention', p)
            plan.conv(ops.conv_params(W[f'{b}.{i}.fn.to_out.0'], att_pl, H, Wd, res1=x, alpha=1.0, out_f32=out))

        def channel_attention(b, i, x, out, grid):
            norm(f'{b}.{i}.norm', x, CONV_LN_EPS)
            plan.conv(ops.conv_params(W[f'{b}.{i}.fn.qkv'], a_pl, H, Wd, out=qkv_pl))
            dwconv(W[f'{b}.{i}.fn.qkv_dwconv'], qkv_pl, 3 * ap, qkv2_pl, L.ACT_NONE)
            p = attn_params(qkv2_pl, grid)
            p.temperature, p.workspace = W[f'{b}.{i}.fn.temperature'].data_ptr(), ws_attn.data_ptr()
            plan.launch('rsa_omni_channel_attention', p, kernels=3 if grid else 1)  # window mode: one launch per call
            plan.conv(ops.conv_params(W[f'{b}.{i}.fn.project_out'], att_pl, H, Wd, res1=x, alpha=1.0, out_f32=out))

        def ffn(b, i, x, out, planes_out=None):
            norm(f'{b}.{i}.norm', x, CONV_LN_EPS)
            plan.conv(ops.conv_params(W[f'{b}.{i}.fn.project_in'], a_pl, H, Wd, out=ffn_pl))
            gp = L.GeluGateDwConvParams()
            gp.batch, gp.H, gp.W, gp.planes, gp.fmt = n, H, Wd, cp, fmt
            ffn_pl.bind(gp, 'in')
            gp.weight = W[f'{b}.{i}.fn.dwconv'].data_ptr()
            mid_pl.bind(gp, 'out')
            plan.launch('rsa_gelu_gate_dwconv', gp)
            plan.conv(ops.conv_params(W[f'{b}.{i}.fn.project_out'], mid_pl, H, Wd, res1=x, alpha=1.0, out_f32=out, out=planes_out))

        def esa(g, x):
            e = f'residual_layer.{g}.esa'
            plan.conv(ops.conv_params(W[f'{e}.conv1'], a_pl, H, Wd, out_f32=c1f))
            for name, src, dst, hi, wi, ho, wo, stride, pad in ((f'{e}.conv2', c1f, c2f, H, Wd, H2, W2, 2, 0), (None, c2f, pmf, H2, W2, Hc, Wc, 0, 0),
                                                               (f'{e}.conv3', pmf, c3f, Hc, Wc, Hc, Wc, 1, 1)):  # fmt: skip
                if name is None:
                    plan.launch('rsa_esa_maxpool', dict(in_=c2f, batch=n, C=f, H=H2, W=W2, out=pmf))
                    continue
                cpar = L.EsaConvParams()
                cpar.batch, cpar.H, cpar.W, cpar.Hout, cpar.Wout, cpar.cin, cpar.cout, cpar.stride, cpar.pad = n, hi, wi, ho, wo, f, f, stride, pad
                cpar.in_, cpar.weight, cpar.bias, cpar.out = src.data_ptr(), W[name][0].data_ptr(), W[name][1].data_ptr(), dst.data_ptr()
                plan.launch('rsa_esa_conv3x3', cpar)
            wf, bf, w4, b4 = W[f'{e}.apply']
            apar = L.EsaApplyParams()
            apar.batch, apar.H, apar.W, apar.C, apar.f, apar.Hc, apar.Wc, apar.fmt = n, H, Wd, c, f, Hc, Wc, fmt
            apar.x, apar.c1, apar.c3, apar.out = x.data_ptr(), c1f.data_ptr(), c3f.data_ptr(), x.data_ptr()
            apar.wf, apar.bf, apar.w4, apar.b4 = wf.data_ptr(), bf.data_ptr(), w4.data_ptr(), b4.data_ptr()
            s_pl.bind(apar, 'out')
            plan.launch('rsa_esa_apply', apar)

        plan.conv(ops.conv_params(W['input'], x_pl, H, Wd, out_f32=first, out=s_pl))
        g_in = first
        for g in range(self.res_num):
            cur = g_in
            for j in range(self.block_num):
                b = f'residual_layer.{g}.residual_layer.{j}.layer'
                for kind, i, grid in (('m', 0, 0), ('w', 2, 0), ('f', 4, 0), ('c', 5, 0), ('f', 6, 0), ('w', 8, 1), ('f', 10, 0), ('c', 11, 1), ('f', 12, 0)):
                    nxt = next(m for m in pool if m is not cur and m is not g_in)
                    if kind == 'm':
                        mbconv(b, cur, nxt)
                    elif kind == 'w':
                        window_attention(b, i, cur, nxt, grid)
                    elif kind == 'c':
                        channel_attention(b, i, cur, nxt, grid)
                    else:  # the last FFN of a block also writes the stream as planes: the next MBConv or the group's 1x1 reads them
                        ffn(b, i, cur, nxt, s_pl if i == 12 else None)
                    cur = nxt
            out = next(m for m in pool if m is not cur and m is not g_in)
            plan.conv(ops.conv_params(W[f'residual_layer.{g}.residual_layer.{self.block_num}'], s_pl, H, Wd, res1=g_in, alpha=1.0, out_f32=out, out=a_pl))
            esa(g, out)
            g_in = out
        fe = plan.planes(n, cp, H, Wd, with_lo)
        plan.conv(ops.conv_params(W['output'], s_pl, H, Wd, res1=first, alpha=1.0, out=fe))
        y = plan.output((n, self.out_ch, H * s, Wd * s), dtype, crop=(h0 * s, w0 * s))
        plan.conv(ops.conv_params(W['up.0'], fe, H, Wd, out_nchw=y, pixel_shuffle=s))
        return set_input
