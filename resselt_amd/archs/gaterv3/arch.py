"""GateRV3 on the MI355X engine (reference module: ``resselt/archs/gaterv3/arch.py:705-802``), EVAL-mode semantics.

A x1..x4 restoration U-Net of ``MetaGated`` blocks with a SPAN side branch.  L = len(enc_blocks) levels; level j runs ``dim 2^j`` channels at
1 / 2^j of the padded input, the latent stage ``dim 2^L`` channels at 1 / 2^L.  The residual stream between blocks is an f32 map.

MetaGated (arch.py:635-668), ten kernels in nine launch steps:

  rsa_rmsnorm (f32 stream -> planes)            local.0: x / (rms + eps) * scale + offset
  -> local.1, a 1x1 convolution to 2 w channels
  -> rsa_gaterv3_local_gate                     local.2 (3x3, groups = w: 2 in / 2 out per group) + SimpleGate, s as planes + its tile sums
  -> rsa_gaterv3_sca_apply (two kernels)        the mean finished in tile order, a = gamma0 * sca(mean), the stream  s * a + short
  -> rsa_rmsnorm -> fc1 (1x1) -> rsa_gated_dwconv (mish(g) * cat(i, Inception(c))) -> fc2 (1x1) + Mish, an f32 map
  -> rsa_group_norm_apply with unit statistics  glob(x) * gamma1 + x: the next stream, and planes where a convolution reads it

The Inception step (identity | dw 3x3 | dw 1x11 | dw 11x1 on gc = w / 8 channels each) takes fc1's rows re-laid out onto whole planes at load
(``archs/mosr/arch.py: gate_layout``), as MoSRv2's does.  A latent block (GatedCNNBlock, no residual) is rsa_rmsnorm -> fc1 -> gate -> fc2 +
Mish; with ``attention`` the token mixer is the 16-head transposed attention: qkv (1x1) -> rsa_dwconv3x3 -> rsa_gaterv3_channel_attention
(three kernels) -> project_out (1x1) written over c's planes of fc1's output, and the gate has no convolution segment.

Down = 3x3 convolution (f32 map) + rsa_pixel_unshuffle2.  Up = 3x3 convolution stored through depth-to-space + the layout kernel that
writes its planes INTO the decoder's concatenation buffer, whose other half the encoder's last block of that level wrote; ``shor`` (1x1)
reads the concatenation without a copy.  The SPAN branch is ``engine/spanblocks.py``'s chain on in_to_dim's output (every Conv3XC folded
once at load in f32 from ``conv.*`` / ``sk``, which win over the stored ``eval_conv.*``); its last 1x1 takes the decoder's stream as its
residual, so ``x + sisr`` costs no launch.  Head: a 3x3 convolution (x1) or ``engine/uniupsample.py``'s ``Head`` (UniUpsampleV3's first five
modes); then rsa_gaterv3_shortcut adds ``gamma * nearest(inp)`` on the cropped output, reading the caller's unpadded input.

Eval mode: the reference's loader returns the module in training mode, where a Conv3XC is conv(pad0(x)) + sk(x); ``model.eval()`` computes
its fold.  The engine computes the fold, as SPAN's and EIMN's do; the two agree to rounding, the border ring included (the first 1x1's bias
reaches the zero-padded ring in both): tests/gaterv3_oracle.py computes the unfolded form and meets the eval-mode fixtures.
``sca`` and the attention span the whole padded tensor (``global_statistics``): a tile computes what the reference computes on that tile.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import lib_gaterv3 as LG3
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.gatedunet import GatedUNetBlocks, _gated_cnn_shapes, _meta_gated_shapes, gate_groups, hidden_of, unit_stats  # noqa: F401  (gate_groups: what the tests import from here)
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.spanblocks import SpabChain, fold_conv3xc
from ...engine.tensors import PF_BF16, Planes
from ...engine.uniupsample import SAMPLE_MODS, SAMPLE_MODS3, Head, OwnMetaUpsample
from ..mosr.arch import _conv_weights

HEADS = 16
MAX_WIDTH = 512  # dim * 2^L: rsa_gaterv3_local_gate and the attention take at most 512 channels
MAX_HEAD_DIM = 64


def _conv3xc_shapes(s: ParamShapes, name: str, c: int, bias: bool, gain: int) -> None:
    g = gain * c
    for sub, (co, ci, k) in (('sk', (c, c, 1)), ('conv.0', (g, c, 1)), ('conv.1', (g, g, 3)), ('conv.2', (c, g, 1)), ('eval_conv', (c, c, 3))):
        s[f'{name}.{sub}.weight'] = (co, ci, k, k)
        if bias:
            s[f'{name}.{sub}.bias'] = (co,)


def _attention_shapes(s: ParamShapes, t: str, w: int) -> None:
    s[f'{t}.temperature'] = (HEADS, 1, 1)
    s[f'{t}.qkv.weight'] = (3 * w, w, 1, 1)
    s[f'{t}.qkv_dwconv.weight'], s[f'{t}.qkv_dwconv.bias'] = (3 * w, 1, 3, 3), (3 * w,)
    s[f'{t}.project_out.weight'] = (w, w, 1, 1)


def trunk_shapes(in_ch: int, dim: int, enc_blocks, dec_blocks, num_latent: int, attention: bool, span_blocks: int) -> ParamShapes:
    """Every parameter in front of ``dim_to_in`` in the order of the reference module's ``state_dict()`` (a module's own parameters come
    before its children's: ``gamma`` first, ``gamma0`` / ``gamma1`` at the head of a MetaGated, ``temperature`` at the head of an Attention)."""
    s = ParamShapes()
    L_ = len(enc_blocks)
    s['gamma'] = (1, in_ch, 1, 1)
    s.conv('in_to_dim', dim, in_ch, 3)
    for j, nb in enumerate(enc_blocks):
        w = dim << j
        for i in range(nb):
            _meta_gated_shapes(s, f'gater_encode.{j}.gated.{i}', w)
        s[f'gater_encode.{j}.scale.0.weight'] = (w // 2, w, 3, 3)
    for name in ['span_block0'] + [f'span_n_b.{i}' for i in range(span_blocks)] + ['span_end']:
        for r in ('c1_r', 'c2_r', 'c3_r'):
            _conv3xc_shapes(s, f'{name}.{r}', dim, False, 2)
    _conv3xc_shapes(s, 'sisr_end_conv', dim, True, 1)  # (gain1 = 1 here, 2 in the SPABs)
    s.conv('sisr_cat_conv', dim, 4 * dim, 1)
    for i in range(num_latent):
        _gated_cnn_shapes(s, f'latent.{i}', dim << L_, _attention_shapes if attention else None)
    for i, nb in enumerate(dec_blocks):
        wb = dim << (len(dec_blocks) - i)
        s[f'decode.{i}.scale.0.weight'] = (2 * wb, wb, 3, 3)
        for k in range(nb):
            _meta_gated_shapes(s, f'decode.{i}.gated.{k}', wb // 2)
        s.conv(f'decode.{i}.shor', wb // 2, wb, 1)
    return s


class _Chain(SpabChain):
    """The SPAB chain whose last 1x1 adds a residual stream: ``sisr_cat_conv(cat) + x``."""

    def run_add(self, names: dict, cat: Planes, xf, res, out: Planes, out_f32) -> None:
        pf = self.pf
        f_b1, f_a, f_b = self.f32
        self.spab(names['first'], cat, 0, xf, cat, 2 * pf, f_b1)
        cur, cur_off, cur_f = cat, 2 * pf, f_b1
        for i, name in enumerate(names['middle']):
            nxt, nf = self.ping[i & 1], (f_a, f_b)[i & 1]
            self.spab(name, cur, cur_off, cur_f, nxt, 0, nf)
            cur, cur_off, cur_f = nxt, 0, nf
        end_out = self.ping[len(names['middle']) & 1]
        self.spab(names['end'], cur, cur_off, cur_f, end_out, 0, None, out1=(cat, 3 * pf))
        self._conv(names['conv_2'], end_out, out=cat, out_plane_off=pf)
        self.plan.conv(ops.conv_params(self.W[names['conv_cat']], cat, self.h, self.w, cin_planes=4 * pf, res1=res, alpha=1.0, out=out, out_f32=out_f32))


class GateRV3(GatedUNetBlocks, OwnMetaUpsample, EngineModule):
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')
    global_statistics = True  # sca's mean and the attention span the whole padded tensor: a tile computes what the reference computes on that tile

    def __init__(self, in_ch: int = 3, dim: int = 32, enc_blocks=(2, 2, 4, 8), dec_blocks=(2, 2, 2, 2), num_latent: int = 12, scale: int = 1,
                 upsample: str = 'pixelshuffle', upsample_mid_dim: int = 32, end_gamma_init: float = 1, attention: bool = False, span_blocks: int = 4,
                 end_kernel: int = 3, **kwargs) -> None:  # fmt: skip
        super().__init__()
        in_ch, dim, scale, num_latent, span_blocks = int(in_ch), int(dim), int(scale), int(num_latent), int(span_blocks)
        enc_blocks, dec_blocks = tuple(int(b) for b in enc_blocks), tuple(int(b) for b in dec_blocks)
        if len(dec_blocks) != len(enc_blocks):
            raise NotImplementedError(f'GateRV3: {len(dec_blocks)} decoder levels for {len(enc_blocks)} encoder levels: the reference builds such a '
                                      'module and raises in forward (the skip connections do not pair up)')  # fmt: skip
        levels = len(enc_blocks)
        if levels < 1 or min(enc_blocks + dec_blocks) < 1 or num_latent < 1 or span_blocks < 0:
            raise NotImplementedError(f'GateRV3: every level and the latent stage need at least one block (got {enc_blocks}, {num_latent}, {dec_blocks})')
        if attention and (dim << levels) % HEADS:
            raise NotImplementedError(f'GateRV3: attention needs a latent width divisible by {HEADS} heads (got {dim << levels}; the reference asserts)')
        if attention and (dim << levels) // HEADS > MAX_HEAD_DIM:
            raise NotImplementedError(f'GateRV3: head_dim {(dim << levels) // HEADS} exceeds {MAX_HEAD_DIM}')
        if dim % 8 or dim < 8:
            raise NotImplementedError(f'GateRV3: dim must be a multiple of 8 (got {dim})')
        if dim << levels > MAX_WIDTH:
            raise NotImplementedError(f'GateRV3: the latent width dim * 2^levels = {dim << levels} exceeds {MAX_WIDTH}')
        if in_ch < 1 or in_ch > 8:
            raise NotImplementedError(f'GateRV3: 1 to 8 input channels are built (got {in_ch})')
        if scale != 1:
            if upsample not in SAMPLE_MODS3:
                raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS3}')
            if upsample == 'conv':
                raise NotImplementedError(f"GateRV3: the 'conv' head does not upsample, so above x1 (got x{scale}) the reference's forward raises: its "
                                          'shortcut is scale times the size of the head output')  # fmt: skip
            if upsample not in SAMPLE_MODS:
                raise NotImplementedError(f'GateRV3: the {upsample} head is not built (conv, pixelshuffledirect, pixelshuffle, nearest+conv and dysample are)')
        self.in_ch, self.dim, self.enc_blocks, self.dec_blocks, self.num_latent = in_ch, dim, enc_blocks, dec_blocks, num_latent
        self.scale, self.upsample, self.mid_dim, self.attention, self.span_blocks, self.end_kernel = scale, upsample, int(upsample_mid_dim), bool(attention), span_blocks, int(end_kernel)
        self.levels, self.pad = levels, 1 << levels
        shapes = trunk_shapes(in_ch, dim, enc_blocks, dec_blocks, num_latent, self.attention, span_blocks)
        buffers: dict = {}
        if scale != 1:
            self.up = Head('dim_to_in', upsample, scale, dim, in_ch, self.mid_dim, end_kernel=self.end_kernel, version=3)
            self.up.shapes(shapes, buffers, whole_planes='GateRV3')
        else:
            self.up = None
            shapes.conv('dim_to_in', in_ch, dim, 3)
        build_param_tree(self, shapes, buffers)
        with torch.no_grad():
            self.gamma.fill_(float(end_gamma_init))

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """As the reference's override (arch.py:766-771): the module's own MetaUpsample buffer wins, a missing ``gamma`` means the module's."""
        state_dict = dict(state_dict)
        if 'gamma' not in state_dict:
            state_dict['gamma'] = self.gamma.detach()
        if self.up is None:
            return EngineModule.load_state_dict(self, state_dict, strict=strict, assign=assign)
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # ---------------------------------------------------------------- accounting
    def meta_gated_count(self) -> int:
        return sum(self.enc_blocks) + sum(self.dec_blocks)

    def macs_per_input_pixel(self) -> int:
        """Multiply-accumulates per pixel of the padded input, each layer at its own resolution (the attention's two d x d products included)."""
        from fractions import Fraction

        d = self.dim

        def gated(w, att):
            h = hidden_of(w)
            mix = (3 * w * w + 27 * w + w * w + 2 * w * (w // HEADS)) if att else (9 + 22) * int(w * 0.125)
            return w * 2 * h + h * w + mix

        def meta(w):
            return w * 2 * w + 18 * 2 * w + w + gated(w, False)

        total = Fraction(9 * self.in_ch * d + (3 * (self.span_blocks + 2) + 1) * 9 * d * d + 4 * d * d)
        for j, nb in enumerate(self.enc_blocks):
            w, px = d << j, Fraction(1, 4**j)
            total += (nb * meta(w) + 9 * w * (w // 2)) * px
        total += self.num_latent * gated(d << self.levels, self.attention) * Fraction(1, 4**self.levels)
        for i, nb in enumerate(self.dec_blocks):
            wb = d << (self.levels - i)
            total += 9 * wb * 2 * wb * Fraction(1, 4 ** (self.levels - i)) + (wb * (wb // 2) + nb * meta(wb // 2)) * Fraction(1, 4 ** (self.levels - i - 1))
        total += self.up.macs() if self.up is not None and self.up.layers else 9 * d * self.in_ch
        return int(total)

    def expected_launches(self) -> int:
        """Kernels per forward (DESIGN.md section 27's table), the head excluded."""
        latent = 10 if self.attention else 4
        span = 3 * (self.span_blocks + 2) + 2
        return 1 + 10 * self.meta_gated_count() + 2 * self.levels + latent * self.num_latent + 3 * self.levels + span + 1

    # ---------------------------------------------------------------- weights
    def _mixer_pack(self, blk, sd, t, w, products, device) -> None:
        own = lambda v: v.to(torch.float32).contiguous().clone()  # noqa: E731  (an allocation of its own: 16-byte aligned)
        blk['qkv'] = ops.ConvWeights.from_oihw(sd[f'{t}.qkv.weight'], None, products, device=device)
        blk['proj'] = ops.ConvWeights.from_oihw(sd[f'{t}.project_out.weight'], None, products, device=device)
        blk['dw'] = (own(sd[f'{t}.qkv_dwconv.weight'].reshape(3 * w, 9)), own(sd[f'{t}.qkv_dwconv.bias']))
        blk['temperature'] = own(sd[f'{t}.temperature'].reshape(-1))

    def span_names(self) -> dict:
        return dict(first='span_block0', middle=[f'span_n_b.{i}' for i in range(self.span_blocks)], end='span_end', conv_2='sisr_end_conv', conv_cat='sisr_cat_conv')

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        cw = lambda name, bias=True: ops.ConvWeights.from_oihw(sd[f'{name}.weight'], sd[f'{name}.bias'] if bias else None, products, device=device)  # noqa: E731
        dim = self.dim
        W: dict = {'in_to_dim': cw('in_to_dim'), 'sisr_cat_conv': cw('sisr_cat_conv')}
        for j, nb in enumerate(self.enc_blocks):
            for i in range(nb):
                self._pack_meta(W, sd, f'gater_encode.{j}.gated.{i}', dim << j, products, device)
            W[f'gater_encode.{j}.scale.0'] = cw(f'gater_encode.{j}.scale.0', False)
        for i in range(self.num_latent):
            blk: dict = {}
            self._pack_gated(blk, sd, f'latent.{i}', dim << self.levels, self.attention, products, device)
            W[f'latent.{i}'] = blk
        for i, nb in enumerate(self.dec_blocks):
            W[f'decode.{i}.scale.0'] = cw(f'decode.{i}.scale.0', False)
            W[f'decode.{i}.shor'] = cw(f'decode.{i}.shor')
            for k in range(nb):
                self._pack_meta(W, sd, f'decode.{i}.gated.{k}', dim << (self.levels - i - 1), products, device)
        # the SPAN branch: every Conv3XC folded once (conv.* and sk win over the stored eval_conv.*); the SPABs' have no biases
        names = self.span_names()
        for spab in [names['first']] + names['middle'] + [names['end']]:
            for r in ('c1_r', 'c2_r', 'c3_r'):
                p = f'{spab}.{r}'
                zb = {f'{p}.{sub}.bias': torch.zeros(sd[f'{p}.{sub}.weight'].shape[0]) for sub in ('sk', 'conv.0', 'conv.1', 'conv.2')}
                w, b = fold_conv3xc({**sd, **zb}, p)
                W[p] = ops.ConvWeights.from_oihw(w, b, products, device=device)
        w, b = fold_conv3xc(sd, 'sisr_end_conv')
        W['sisr_end_conv'] = ops.ConvWeights.from_oihw(w, b, products, device=device)
        W['zeros'] = torch.zeros(dim << self.levels, dtype=torch.float32, device=device)
        W['gamma'] = sd['gamma'].reshape(-1).contiguous().clone()
        if self.up is not None:
            self.up.pack(W, sd, products, device)
        else:
            W['head0'] = cw('dim_to_in')
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    # ---------------------------------------------------------------- plan
    def _mixer_bufs(self, plan: Plan, b, n, H, Wd, w, with_lo) -> None:
        b['qkv'], b['qkv2'], b['attn'] = plan.planes(n, 3 * w // 8, H, Wd, with_lo), plan.planes(n, 3 * w // 8, H, Wd, with_lo), plan.planes(n, w // 8, H, Wd, with_lo)
        nbytes = int(L.load().rsa_gaterv3_attn_workspace_bytes(n, H, Wd, HEADS, w // HEADS))
        if nbytes <= 0:
            raise RuntimeError('rsa_gaterv3_attn_workspace_bytes refused the latent grid')
        b['ws'] = torch.empty(nbytes // 4, dtype=torch.float32, device=plan.device)
        plan.keep.append(b['ws'])

    def _mixer(self, plan: Plan, blk, n, H, Wd, w, F_pl: Planes, c0: int, bufs) -> None:
        """The 16-head transposed attention on c's planes of fc1's output: qkv (1x1) -> rsa_dwconv3x3 -> rsa_gaterv3_channel_attention ->
        project_out (1x1) written over c's planes."""
        cp, d = w // 8, w // HEADS
        Q, Q2, A, ws = bufs['qkv'], bufs['qkv2'], bufs['attn'], bufs['ws']
        unit = 16 * (2 if Q.lo is not None else 1)
        px = n * H * Wd
        plan.conv(ops.conv_params(blk['qkv'], F_pl, H, Wd, in_plane0=c0, out=Q))
        dp = L.DwConvParams()
        dp.batch, dp.H, dp.W, dp.planes, dp.act, dp.fmt = n, H, Wd, 3 * cp, L.ACT_NONE, Q.fmt
        Q.bind(dp, 'in')
        dp.weight, dp.bias = blk['dw'][0].data_ptr(), blk['dw'][1].data_ptr()
        Q2.bind(dp, 'out')
        plan.launch('rsa_dwconv3x3', dp, meta=dict(kernel='rsa_dwconv3x3', flop=2 * px * 9 * 3 * w, bytes=px * 6 * cp * unit))
        ap = LG3.AttnParams()
        ap.batch, ap.H, ap.W, ap.C, ap.heads, ap.head_dim, ap.fmt = n, H, Wd, w, HEADS, d, Q2.fmt
        Q2.bind(ap, 'qkv')
        A.bind(ap, 'out')
        ap.temperature, ap.workspace, ap.workspace_bytes = blk['temperature'].data_ptr(), ws.data_ptr(), ws.numel() * 4
        chunks = (H * Wd + LG3.TOKEN_CHUNK - 1) // LG3.TOKEN_CHUNK
        rec = 4 * HEADS * (d * d + 2 * d)
        # byte model: q and k read once, a record per chunk written and read, A written and read, v read once, the output planes written
        plan.launch('rsa_gaterv3_channel_attention', ap, kernels=3,
                    meta=dict(kernel='rsa_gaterv3_channel_attention', flop=4 * px * w * d, bytes=px * 4 * cp * unit + n * (2 * chunks * rec + 8 * HEADS * d * d)))  # fmt: skip
        plan.conv(ops.conv_params(blk['proj'], A, H, Wd, out=F_pl, out_plane_off=c0))

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):  # noqa: C901
        n, c, h0, w0 = x_shape
        if c != self.in_ch:
            raise RuntimeError(f'model expects {self.in_ch} input channels, got {c}')
        P, s, dim = self.pad, self.scale, self.dim
        Hp, Wp = h0 + (P - h0 % P) % P, w0 + (P - w0 % P) % P
        if Hp - h0 >= h0 or Wp - w0 >= w0:
            raise RuntimeError(f'Padding size should be less than the corresponding input dimension (a {h0}x{w0} input cannot be reflect-padded '
                               f'to a multiple of {P})')  # fmt: skip
        with_lo = products == 3
        cache: dict = {}
        pd = dim // 8
        x_pl = plan.planes(n, 1, Hp, Wp, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)  # check_img_size's bottom / right reflect pad, fused

        stats = unit_stats(plan, n)
        chain = _Chain(plan, W, n, Hp, Wp, dim, L.ACT_SILU, with_lo)
        cat_s = chain.new_cat()  # [x | sisr_end_conv | span_block0 | span_end's out1]
        x0 = plan.f32map(n, dim, Hp, Wp)
        plan.conv(ops.conv_params(W['in_to_dim'], x_pl, Hp, Wp, out=cat_s, out_f32=x0))
        cats, cur, H, Wd = self._encoder(plan, W, 'gater_encode', n, Hp, Wp, x0, with_lo, cache, stats)
        prev = self._latent(plan, W, n, H, Wd, cur, self.attention, with_lo, cache)
        cur = self._decoder(plan, W, n, H, Wd, prev, cats, with_lo, cache, stats)
        # the SPAN branch on in_to_dim's output; its last 1x1 adds the decoder's stream: x + sisr, the planes the head reads
        fe = plan.planes(n, pd, Hp, Wp, with_lo)
        fe32 = plan.f32map(n, dim, Hp, Wp) if self.up is not None and self.up.needs_f32_input(W) else None
        chain.run_add(self.span_names(), cat_s, x0, cur, fe, fe32)
        y = plan.output((n, self.in_ch, Hp * s, Wp * s), dtype, crop=(h0 * s, w0 * s))
        if self.up is not None:
            self.up.emit(plan, W, fe, fe32, y, with_lo)
        else:
            plan.conv(ops.conv_params(W['head0'], fe, Hp, Wp, out_nchw=y))
        sp = LG3.ShortcutParams()
        sp.batch, sp.C, sp.h, sp.w, sp.scale, sp.out_H, sp.out_W, sp.dtype = n, self.in_ch, h0, w0, s, Hp * s, Wp * s, ops.rsa_dtype(dtype)
        sp.x, sp.gamma, sp.out = plan.input_ref(x_shape, dtype).data_ptr(), W['gamma'].data_ptr(), y.data_ptr()
        esize = torch.empty((), dtype=dtype).element_size()
        plan.launch('rsa_gaterv3_shortcut', sp, meta=dict(kernel='rsa_gaterv3_shortcut', flop=2 * n * c * h0 * w0 * s * s,
                                                          bytes=n * c * h0 * w0 * esize * (1 + 2 * s * s)))  # fmt: skip
        return set_input
