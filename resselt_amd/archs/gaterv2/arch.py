"""GateRv2 on the MI355X engine (reference module: ``resselt/archs/gaterv2/arch.py:394-470``).  Nothing in the reference module differs
between training and eval mode; the engine computes what both compute.

A x1..x4 restoration U-Net of ``MetaGated`` blocks, the middle model of the ``gater`` family.  L = len(enc_blocks) levels; level j runs
``dim 2^j`` channels at 1 / 2^j of the padded input, the latent stage ``dim 2^L`` channels at 1 / 2^L.  MetaGated, Down, Up and ``shor`` are
GateRV3's, line for line, and are built by the same code (``engine/gatedunet.py``).  What is GateRv2's own:

* the latent token mixer, always on: an l2-normalised linear attention with C / 16 query / key channels and C value channels
  (arch.py:215-250).  A latent block (GatedCNNBlock, no residual) is seven launch steps:

    rsa_rmsnorm -> fc1 (1x1) -> the fused q | k | v 1x1 reading c's planes of fc1's output (the rows of query_conv, key_conv and value_conv
    concatenated at load, q and k zero-padded to whole planes) -> rsa_gaterv2_linear_attention (three kernels) writing over c's planes
    -> rsa_gated_dwconv with one passthrough segment -> fc2 (1x1) + Mish -> the stream hand-over (fc2's f32 map IS the next stream);

* the output: ``dim_to_in(x) + short_to_dim(inp)`` -> ``upsample`` -> crop.  At x1 ``dim_to_in`` is a 3x3 convolution to ``in_ch`` and the
  padded input itself is added (rsa_bilinear_add at scale 1 on the cropped output).  Above x1 ``short_to_dim`` is a ConvBlock (3x3 + Mish,
  3x3 + Mish, plus a 1x1 of the input): the 1x1 runs first, and the second 3x3 + Mish adds it AND the decoder's stream as its two
  post-activation residuals, so both sums cost no launch; ``upsample`` is UniUpsample v1 (``engine/uniupsample.py``'s ``Head``; its
  DySample has no front convolution and a 1x1 end convolution);
* no SPAN branch and no ``gamma`` shortcut;
* a latent width of up to 1024 (the default model: 48 * 2^4 = 768), while a MetaGated runs at most ``dim 2^(L - 1)`` <= 512 channels.

Two defects of the reference, and what the engine does instead (tests/golden/gaterv2_probe.npz records both):

* its loader reads ``state['to_img.MetaUpsample']`` where the state dict has ``upsample.MetaUpsample`` and raises ``KeyError``: it loads x1
  checkpoints only.  The engine's loader reads ``upsample.MetaUpsample``;
* the module sets ``self.scale = 1`` whatever scale it is given, so a module built with ``scale > 1`` returns the top-left H x W corner of
  the upscaled image.  The engine returns the full ``H scale x W scale`` image.  A 'conv' head does not upsample: above x1 the output is the
  padded map cropped to at most ``H scale x W scale``.

``sca`` and the attention span the whole padded tensor (``global_statistics``): a tile computes what the reference computes on that tile.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import lib_gaterv2 as LG2
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.gatedunet import MAX_META_WIDTH, GatedUNetBlocks, _gated_cnn_shapes, _meta_gated_shapes, _view, hidden_of, unit_stats
from ...engine.paramtree import ParamShapes, build_param_tree
from ...engine.tensors import PF_BF16, Planes
from ...engine.uniupsample import SAMPLE_MODS, Head, OwnMetaUpsample
from ..mosr.arch import _conv_weights

QK_DIV = 16  # Attention(in_places, scale=16): m = C // 16 query / key channels
ATTN_EPS = 1e-6
MAX_LATENT_WIDTH = 1024  # rsa_gaterv2_linear_attention's C; no convolution, rsa_rmsnorm or rsa_gated_dwconv path has a width limit below it


def _attention_shapes(s: ParamShapes, t: str, w: int) -> None:
    m = w // QK_DIV
    s.conv(f'{t}.query_conv', m, w, 1)
    s.conv(f'{t}.key_conv', m, w, 1)
    s.conv(f'{t}.value_conv', w, w, 1)


def trunk_shapes(in_ch: int, dim: int, enc_blocks, dec_blocks, num_latent: int) -> ParamShapes:
    """Every parameter in front of ``dim_to_in`` / ``short_to_dim`` in the order of the reference module's ``state_dict()``."""
    s = ParamShapes()
    s.conv('in_to_dim', dim, in_ch, 3)
    for j, nb in enumerate(enc_blocks):
        w = dim << j
        for i in range(nb):
            _meta_gated_shapes(s, f'encode.{j}.gated.{i}', w)
        s[f'encode.{j}.scale.0.weight'] = (w // 2, w, 3, 3)
    for i in range(num_latent):
        _gated_cnn_shapes(s, f'latent.{i}', dim << len(enc_blocks), _attention_shapes)
    for i, nb in enumerate(dec_blocks):
        wb = dim << (len(dec_blocks) - i)
        s[f'decode.{i}.scale.0.weight'] = (2 * wb, wb, 3, 3)
        for k in range(nb):
            _meta_gated_shapes(s, f'decode.{i}.gated.{k}', wb // 2)
        s.conv(f'decode.{i}.shor', wb // 2, wb, 1)
    return s


class GateRV2(GatedUNetBlocks, OwnMetaUpsample, EngineModule):
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')
    global_statistics = True  # sca's mean and the attention span the whole padded tensor: a tile computes what the reference computes on that tile

    def __init__(self, in_ch: int = 3, dim: int = 48, enc_blocks=(2, 2, 4, 6), dec_blocks=(2, 2, 2, 2), num_latent: int = 10, scale: int = 1,
                 upsample: str = 'pixelshuffledirect', upsample_mid_dim: int = 32, **kwargs) -> None:  # fmt: skip
        super().__init__()
        in_ch, dim, scale, num_latent = int(in_ch), int(dim), int(scale), int(num_latent)
        enc_blocks, dec_blocks = tuple(int(b) for b in enc_blocks), tuple(int(b) for b in dec_blocks)
        if len(dec_blocks) != len(enc_blocks):
            raise NotImplementedError(f'GateRv2: {len(dec_blocks)} decoder levels for {len(enc_blocks)} encoder levels: the reference builds such a '
                                      'module and raises in forward (the skip connections do not pair up)')  # fmt: skip
        levels = len(enc_blocks)
        if levels < 1 or min(enc_blocks + dec_blocks) < 1 or num_latent < 1:
            raise NotImplementedError(f'GateRv2: every level and the latent stage need at least one block (got {enc_blocks}, {num_latent}, {dec_blocks})')
        if dim % 8 or dim < 8:
            raise NotImplementedError(f'GateRv2: dim must be a multiple of 8 (got {dim})')
        # (the latent stage is twice as wide as the widest MetaGated, so the first of these two limits is the one a model meets)
        if dim << (levels - 1) > MAX_META_WIDTH:
            raise NotImplementedError(f'GateRv2: the widest MetaGated, dim * 2^(levels - 1) = {dim << (levels - 1)}, exceeds {MAX_META_WIDTH} (rsa_gaterv3_local_gate)')
        if dim << levels > MAX_LATENT_WIDTH:
            raise NotImplementedError(f'GateRv2: the latent width dim * 2^levels = {dim << levels} exceeds {MAX_LATENT_WIDTH} (rsa_gaterv2_linear_attention)')
        if in_ch < 1 or in_ch > 8:
            raise NotImplementedError(f'GateRv2: 1 to 8 input channels are built (got {in_ch})')
        if scale != 1 and upsample not in SAMPLE_MODS:
            raise ValueError(f'An invalid Upsample was selected. Please choose one of {SAMPLE_MODS}')
        self.in_ch, self.dim, self.enc_blocks, self.dec_blocks, self.num_latent = in_ch, dim, enc_blocks, dec_blocks, num_latent
        self.scale, self.upsampler, self.mid_dim = scale, upsample, int(upsample_mid_dim)  # (``upsample`` is the head's sub-module)
        self.levels, self.pad = levels, 1 << levels
        self.latent_width, self.qk = dim << levels, (dim << levels) // QK_DIV
        shapes = trunk_shapes(in_ch, dim, enc_blocks, dec_blocks, num_latent)
        buffers: dict = {}
        if scale != 1:
            shapes.conv('short_to_dim.block.0', dim, in_ch, 3)
            shapes.conv('short_to_dim.block.2', dim, dim, 3)
            shapes.conv('short_to_dim.conv11', dim, in_ch, 1)
            # (UniUpsample of this family gives DySample the features themselves: no mid_dim convolution in front of it)
            self.up = Head('upsample', upsample, scale, dim, in_ch, dim if upsample == 'dysample' else self.mid_dim, version=1, meta_mid_dim=self.mid_dim)
            self.up.shapes(shapes, buffers, whole_planes='GateRv2')
        else:
            self.up = None
            shapes.conv('dim_to_in', in_ch, dim, 3)
        build_param_tree(self, shapes, buffers)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """As the reference's override (arch.py:444-447): the module's own MetaUpsample buffer wins."""
        if self.up is None:
            return EngineModule.load_state_dict(self, dict(state_dict), strict=strict, assign=assign)
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # ---------------------------------------------------------------- accounting
    def meta_gated_count(self) -> int:
        return sum(self.enc_blocks) + sum(self.dec_blocks)

    def macs_per_input_pixel(self) -> int:
        """Multiply-accumulates per pixel of the padded input, each layer at its own resolution (the attention: q | k | v, M and the apply)."""
        from fractions import Fraction

        d = self.dim

        def gated(w, att):
            h = hidden_of(w)
            m = w // QK_DIV
            mix = (w * (2 * m + w) + 2 * m * w) if att else (9 + 22) * int(w * 0.125)
            return w * 2 * h + h * w + mix

        def meta(w):
            return w * 2 * w + 18 * 2 * w + w + gated(w, False)

        total = Fraction(9 * self.in_ch * d)
        for j, nb in enumerate(self.enc_blocks):
            w, px = d << j, Fraction(1, 4**j)
            total += (nb * meta(w) + 9 * w * (w // 2)) * px
        total += self.num_latent * gated(d << self.levels, True) * Fraction(1, 4**self.levels)
        for i, nb in enumerate(self.dec_blocks):
            wb = d << (self.levels - i)
            total += 9 * wb * 2 * wb * Fraction(1, 4 ** (self.levels - i)) + (wb * (wb // 2) + nb * meta(wb // 2)) * Fraction(1, 4 ** (self.levels - i - 1))
        if self.up is not None:
            total += self.in_ch * d * 10 + 9 * d * d + (self.up.macs() if self.up.layers else 0)
        else:
            total += 9 * d * self.in_ch
        return int(total)

    def expected_launches(self) -> int:
        """Kernels per forward (DESIGN.md section 28's table), the head excluded: in_to_dim, ten per MetaGated, two per Down, eight per latent
        block (the attention is three), three per Up, and the shortcut (x1: the addition of the input; above: the ConvBlock's three)."""
        return 1 + 10 * self.meta_gated_count() + 2 * self.levels + 8 * self.num_latent + 3 * self.levels + (1 if self.up is None else 3)

    # ---------------------------------------------------------------- weights
    def _mixer_pack(self, blk, sd, t, w, products, device) -> None:
        """query_conv | key_conv | value_conv as ONE 1x1 convolution: the q and the k rows zero-padded to whole planes (zero weight and bias
        rows give exact zeros)."""
        m = w // QK_DIV
        mp8 = (m + 7) // 8 * 8
        wq = torch.zeros((2 * mp8 + w, w, 1, 1), dtype=torch.float32, device=device)
        bq = torch.zeros(2 * mp8 + w, dtype=torch.float32, device=device)
        for row0, name, rows in ((0, 'query_conv', m), (mp8, 'key_conv', m), (2 * mp8, 'value_conv', w)):
            wq[row0 : row0 + rows], bq[row0 : row0 + rows] = sd[f'{t}.{name}.weight'], sd[f'{t}.{name}.bias']
        blk['qkv'] = ops.ConvWeights.from_oihw(wq, bq, products, device=device)
        blk['m'] = m

    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items() if not k.endswith('MetaUpsample')}
        cw = lambda name, bias=True: ops.ConvWeights.from_oihw(sd[f'{name}.weight'], sd[f'{name}.bias'] if bias else None, products, device=device)  # noqa: E731
        dim = self.dim
        W: dict = {'in_to_dim': cw('in_to_dim')}
        for j, nb in enumerate(self.enc_blocks):
            for i in range(nb):
                self._pack_meta(W, sd, f'encode.{j}.gated.{i}', dim << j, products, device)
            W[f'encode.{j}.scale.0'] = cw(f'encode.{j}.scale.0', False)
        for i in range(self.num_latent):
            blk: dict = {}
            self._pack_gated(blk, sd, f'latent.{i}', self.latent_width, True, products, device)
            W[f'latent.{i}'] = blk
        for i, nb in enumerate(self.dec_blocks):
            W[f'decode.{i}.scale.0'] = cw(f'decode.{i}.scale.0', False)
            W[f'decode.{i}.shor'] = cw(f'decode.{i}.shor')
            for k in range(nb):
                self._pack_meta(W, sd, f'decode.{i}.gated.{k}', dim << (self.levels - i - 1), products, device)
        W['zeros'] = torch.zeros(self.latent_width, dtype=torch.float32, device=device)
        if self.up is not None:
            for name in ('short_to_dim.block.0', 'short_to_dim.block.2', 'short_to_dim.conv11'):
                W[name] = cw(name)
            self.up.pack(W, sd, products, device)
        else:
            W['head0'] = cw('dim_to_in')
        if products.fmt != PF_BF16:
            check_fp16_range(_conv_weights(W))
        return W

    # ---------------------------------------------------------------- plan
    def _mixer_bufs(self, plan: Plan, b, n, H, Wd, w, with_lo) -> None:
        m = w // QK_DIV
        b['qkv'], b['attn'] = plan.planes(n, 2 * ((m + 7) // 8) + w // 8, H, Wd, with_lo), plan.planes(n, w // 8, H, Wd, with_lo)
        nbytes = int(L.load().rsa_gaterv2_attn_workspace_bytes(n, H, Wd, w, m))
        if nbytes <= 0:
            raise RuntimeError('rsa_gaterv2_attn_workspace_bytes refused the latent grid')
        b['ws'] = torch.empty(nbytes // 4, dtype=torch.float32, device=plan.device)
        plan.keep.append(b['ws'])

    def _mixer(self, plan: Plan, blk, n, H, Wd, w, F_pl: Planes, c0: int, bufs) -> None:
        """The l2-normalised linear attention on c's planes of fc1's output: q | k | v (one 1x1) -> rsa_gaterv2_linear_attention written
        over c's planes."""
        m, cp = blk['m'], w // 8
        mp = (m + 7) // 8
        Q, ws = bufs['qkv'], bufs['ws']
        unit = 16 * (2 if Q.lo is not None else 1)
        tokens = H * Wd
        plan.conv(ops.conv_params(blk['qkv'], F_pl, H, Wd, in_plane0=c0, out=Q))
        ap = LG2.AttnParams()
        ap.batch, ap.H, ap.W, ap.C, ap.m, ap.fmt, ap.eps = n, H, Wd, w, m, Q.fmt, ATTN_EPS
        Q.bind(ap, 'qkv')
        _view(F_pl, c0, cp).bind(ap, 'out')
        ap.workspace, ap.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        chunks = (tokens + LG2.TOKEN_CHUNK - 1) // LG2.TOKEN_CHUNK
        groups = (w + 63) // 64
        rec = 4 * LG2.record_floats(w, m)
        # byte model: k read once per group of 64 value channels and v once (partial), q once per group (apply), the output planes written
        # once; a record per chunk written and read, the finished record written and read
        plan.launch('rsa_gaterv2_linear_attention', ap, kernels=3,
                    meta=dict(kernel='rsa_gaterv2_linear_attention', flop=n * tokens * (4 * m * w + 6 * m),
                              bytes=n * tokens * unit * (2 * mp * groups + 2 * cp) + n * 2 * (chunks + 1) * rec))  # fmt: skip

    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
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
        x0 = plan.f32map(n, dim, Hp, Wp)
        plan.conv(ops.conv_params(W['in_to_dim'], x_pl, Hp, Wp, out_f32=x0))
        cats, cur, H, Wd = self._encoder(plan, W, 'encode', n, Hp, Wp, x0, with_lo, cache, stats)
        prev = self._latent(plan, W, n, H, Wd, cur, True, with_lo, cache)
        fe = plan.planes(n, pd, Hp, Wp, with_lo)
        if self.up is None:
            # x1: the decoder's last block writes the planes dim_to_in reads; + the padded input over the region that is kept
            self._decoder(plan, W, n, H, Wd, prev, cats, with_lo, cache, stats, out_last=fe)
            y = plan.output((n, self.in_ch, Hp, Wp), dtype, crop=(h0, w0))
            plan.conv(ops.conv_params(W['head0'], fe, Hp, Wp, out_nchw=y))
            bp = L.BilinearAddParams()  # scale 1: every weight exactly 0 or 1
            bp.batch, bp.C, bp.h, bp.w, bp.pad_h, bp.pad_w, bp.scale = n, self.in_ch, h0, w0, Hp, Wp, 1
            bp.dtype = ops.rsa_dtype(dtype)
            bp.out_H, bp.out_W, bp.out_h, bp.out_w = Hp, Wp, h0, w0
            bp.x, bp.out = plan.input_ref(x_shape, dtype).data_ptr(), y.data_ptr()
            plan.launch('rsa_bilinear_add', bp)
            return set_input
        cur = self._decoder(plan, W, n, H, Wd, prev, cats, with_lo, cache, stats)
        # short_to_dim: conv11 first; the second 3x3 + Mish adds it and the decoder's stream after the activation: x + short_to_dim(inp)
        c11 = plan.f32map(n, dim, Hp, Wp)
        plan.conv(ops.conv_params(W['short_to_dim.conv11'], x_pl, Hp, Wp, out_f32=c11))
        t1 = plan.planes(n, pd, Hp, Wp, with_lo)
        plan.conv(ops.conv_params(W['short_to_dim.block.0'], x_pl, Hp, Wp, act=L.ACT_MISH, out=t1))
        fe32 = plan.f32map(n, dim, Hp, Wp) if self.up.needs_f32_input(W) else None
        plan.conv(ops.conv_params(W['short_to_dim.block.2'], t1, Hp, Wp, act=L.ACT_MISH, res1=c11, alpha=1.0, res2=cur, beta=1.0, out=fe, out_f32=fe32))
        if self.upsampler == 'conv':  # does not upsample: the crop is clamped to the padded map
            y = plan.output((n, self.in_ch, Hp, Wp), dtype, crop=(min(Hp, h0 * s), min(Wp, w0 * s)))
        else:
            y = plan.output((n, self.in_ch, Hp * s, Wp * s), dtype, crop=(h0 * s, w0 * s))
        self.up.emit(plan, W, fe, fe32, y, with_lo)
        return set_input
