"""The blocks GateRv2 and GateRV3 share (reference ``archs/gaterv2/arch.py`` and ``archs/gaterv3/arch.py``: RMSNorm, InceptionDWConv2d,
GatedCNNBlock, SimpleGate, MetaGated, Down, Upsample and Block are the same in both, line for line): parameter shapes, weight packing and
the launches of a MetaGated block, of a GatedCNNBlock and of a stage of MetaGated blocks, as a mixin of the family's ``EngineModule``.

MetaGated, ten kernels in nine launch steps:

  rsa_rmsnorm (f32 stream -> planes)            local.0: x / (rms + eps) * scale + offset
  -> local.1, a 1x1 convolution to 2 w channels
  -> rsa_gaterv3_local_gate                     local.2 (3x3, groups = w: 2 in / 2 out per group) + SimpleGate, s as planes + its tile sums
  -> rsa_gaterv3_sca_apply (two kernels)        the mean finished in tile order, a = gamma0 * sca(mean), the stream  s * a + short
  -> rsa_rmsnorm -> fc1 (1x1) -> rsa_gated_dwconv (mish(g) * cat(i, Inception(c))) -> fc2 (1x1) + Mish, an f32 map
  -> rsa_group_norm_apply with unit statistics  glob(x) * gamma1 + x: the next stream, and planes where a convolution reads it

The latent GatedCNNBlock's token mixer is the family's own; the three ``_mixer_*`` hooks and ``mixer_shapes`` are where it plugs in.  With a
mixer the gate has no convolution segment: the mixer writes over c's planes of fc1's output.
"""

from __future__ import annotations

import torch

from ..archs.mosr.arch import gate_layout, pad_dw, relayout_gate
from . import lib as L
from . import lib_gaterv3 as LG3
from . import ops, plk
from .base import Plan
from .paramtree import ParamShapes
from .tensors import PF_BF16, Planes

MAX_META_WIDTH = 512  # rsa_gaterv3_local_gate and rsa_gaterv3_sca_apply take at most 512 channels
RMS_EPS = 1e-6
INCEPTION = (('dwconv_hw', (3, 3)), ('dwconv_w', (1, 11)), ('dwconv_h', (11, 1)))


def _view(p: Planes, plane0: int, planes: int) -> Planes:
    """Planes [plane0, plane0 + planes) of a buffer as a buffer of its own (same storage and strides)."""
    lo = p.lo[:, plane0 : plane0 + planes] if p.has_lo(plane0, planes) else None
    return Planes(p.hi[:, plane0 : plane0 + planes], lo)


def hidden_of(width: int) -> int:
    return int(1.5 * width)


def gate_groups(width: int, att: bool):
    """cat(i, c) of a GatedCNNBlock in channel order: [(channels, kernel shape)], (1, 1) = passthrough."""
    hidden = hidden_of(width)
    if att:
        return [(hidden, (1, 1))]
    gc = int(width * 0.125)
    return [(hidden - 3 * gc, (1, 1))] + [(gc, k) for _, k in INCEPTION]


def _gated_cnn_shapes(s: ParamShapes, b: str, w: int, mixer_shapes=None) -> None:
    """A GatedCNNBlock's parameters; ``mixer_shapes(s, prefix, w)`` adds the token mixer's where it is not the Inception convolution."""
    hidden = hidden_of(w)
    s[f'{b}.norm.scale'], s[f'{b}.norm.offset'] = (w,), (w,)
    s.conv(f'{b}.fc1', 2 * hidden, w, 1)
    if mixer_shapes is not None:
        mixer_shapes(s, f'{b}.token_mix', w)
    else:
        gc = int(w * 0.125)
        for name, (kh, kw) in INCEPTION:
            s[f'{b}.token_mix.{name}.weight'], s[f'{b}.token_mix.{name}.bias'] = (gc, 1, kh, kw), (gc,)
    s.conv(f'{b}.fc2', w, hidden, 1)


def _meta_gated_shapes(s: ParamShapes, b: str, w: int) -> None:
    s[f'{b}.gamma0'], s[f'{b}.gamma1'] = (1, w, 1, 1), (1, w, 1, 1)
    s[f'{b}.local.0.scale'], s[f'{b}.local.0.offset'] = (w,), (w,)
    s.conv(f'{b}.local.1', 2 * w, w, 1)
    s[f'{b}.local.2.weight'], s[f'{b}.local.2.bias'] = (2 * w, 2, 3, 3), (2 * w,)
    s.conv(f'{b}.sca.1', w, w, 1)
    _gated_cnn_shapes(s, f'{b}.glob', w)


def unit_stats(plan: Plan, n: int) -> torch.Tensor:
    """Mean 0 and inverse deviation 1 per image: rsa_group_norm_apply then computes ``x * gamma1 + residual``."""
    stats = torch.zeros((n, 1, 2), dtype=torch.float32, device=plan.device)
    stats[..., 1] = 1.0
    plan.keep.append(stats)
    return stats


class GatedUNetBlocks:
    """Mixin: the packing and the launches of the shared blocks.  A family with a latent token mixer overrides ``_mixer_pack`` (weights into
    ``blk``), ``_mixer_bufs`` (buffers into ``b``) and ``_mixer`` (the launches between fc1 and the gate)."""

    # ---------------------------------------------------------------- the latent token mixer: the family's own
    def _mixer_pack(self, blk, sd, t, w, products, device) -> None:
        raise NotImplementedError

    def _mixer_bufs(self, plan: Plan, b, n, H, Wd, w, with_lo) -> None:
        raise NotImplementedError

    def _mixer(self, plan: Plan, blk, n, H, Wd, w, F_pl: Planes, c0: int, bufs) -> None:
        raise NotImplementedError

    # ---------------------------------------------------------------- weights
    def _pack_gated(self, blk, sd, b, w, att, products, device):
        f32 = torch.float32
        perm, i_planes, segs, planes = gate_layout(gate_groups(w, att))
        w1, b1, w2 = relayout_gate(sd[f'{b}.fc1.weight'], sd[f'{b}.fc1.bias'], sd[f'{b}.fc2.weight'], perm, planes)
        own = lambda t: t.to(f32).contiguous().clone()  # noqa: E731  (an allocation of its own: 16-byte aligned)
        blk['norm'] = (own(sd[f'{b}.norm.scale']), own(sd[f'{b}.norm.offset']))
        # rsa_rmsnorm writes bf16 planes: in the fp16 mode the layers that read them take one bf16 product
        nprod = products if products.fmt == PF_BF16 else 1
        blk['fc1'] = ops.ConvWeights.from_oihw(w1.to(f32), b1.to(f32), nprod, fmt=PF_BF16, device=device)
        blk['fc2'] = ops.ConvWeights.from_oihw(w2.to(f32), sd[f'{b}.fc2.bias'], products, device=device)
        blk['i_planes'], blk['planes'], blk['att'] = i_planes, planes, att
        if att:
            self._mixer_pack(blk, sd, f'{b}.token_mix', w, products, device)
            blk['segs'] = []
        else:
            blk['segs'] = [(pl, kh, kw, *pad_dw(sd[f'{b}.token_mix.{name}.weight'], sd[f'{b}.token_mix.{name}.bias'], pl))
                           for (pl, kh, kw, _, _), (name, _) in zip(segs, INCEPTION)]  # fmt: skip

    def _pack_meta(self, W, sd, b, w, products, device):
        f32 = torch.float32
        own = lambda t: t.to(f32).contiguous().clone()  # noqa: E731
        nprod = products if products.fmt == PF_BF16 else 1
        blk = dict(lnorm=(own(sd[f'{b}.local.0.scale']), own(sd[f'{b}.local.0.offset'])),
                   local1=ops.ConvWeights.from_oihw(sd[f'{b}.local.1.weight'], sd[f'{b}.local.1.bias'], nprod, fmt=PF_BF16, device=device),
                   local2=(own(sd[f'{b}.local.2.weight'].reshape(2 * w, 18)), own(sd[f'{b}.local.2.bias'])),
                   sca=(own(sd[f'{b}.sca.1.weight'].reshape(w, w)), own(sd[f'{b}.sca.1.bias'])),
                   gamma0=own(sd[f'{b}.gamma0'].reshape(-1)), gamma1=own(sd[f'{b}.gamma1'].reshape(-1)))  # fmt: skip
        self._pack_gated(blk, sd, f'{b}.glob', w, False, products, device)
        W[b] = blk

    # ---------------------------------------------------------------- plan
    def _rmsnorm(self, plan: Plan, cur, n, H, Wd, w, norm, N_pl) -> None:
        unit = 16 * (2 if N_pl.lo is not None else 1)
        plan.launch('rsa_rmsnorm', dict(x_f32=cur, batch=n, H=H, W=Wd, C=w, eps=RMS_EPS, scale=norm[0], offset=norm[1], out=N_pl),
                    meta=dict(kernel='rsa_rmsnorm', flop=0, bytes=n * H * Wd * (4 * w + unit * (w // 8))))  # fmt: skip

    def _gate(self, plan: Plan, blk, n, H, Wd, F_pl, M_pl) -> None:
        hp = blk['planes']
        gp = L.GatedDwConvParams()
        gp.batch, gp.H, gp.W, gp.fmt, gp.i_planes, gp.n_segments = n, H, Wd, F_pl.fmt, blk['i_planes'], len(blk['segs'])
        for s, (pl, kh, kw, wt, bt) in enumerate(blk['segs']):
            gp.seg[s].planes, gp.seg[s].kh, gp.seg[s].kw = pl, kh, kw
            gp.seg[s].weight, gp.seg[s].bias = wt.data_ptr(), bt.data_ptr()
        F_pl.bind(gp, 'g')
        F_pl.bind(gp, 'x', hp)
        M_pl.bind(gp, 'out')
        unit = 16 * (2 if F_pl.lo is not None else 1)
        plan.launch('rsa_gated_dwconv', gp, meta=dict(kernel='rsa_gated_dwconv', flop=0, bytes=n * H * Wd * unit * 3 * hp))

    def _bufs(self, plan: Plan, n, H, Wd, w, att, with_lo, cache):
        key = (w, H, Wd, att)
        if key in cache:
            return cache[key]
        hp = gate_layout(gate_groups(w, att))[3]
        b = dict(norm=plan.planes(n, w // 8, H, Wd, with_lo, fmt=PF_BF16), fc1=plan.planes(n, 2 * hp, H, Wd, with_lo), gate=plan.planes(n, hp, H, Wd, with_lo))
        if att:
            self._mixer_bufs(plan, b, n, H, Wd, w, with_lo)
        else:
            b['local'], b['s'] = plan.planes(n, 2 * w // 8, H, Wd, with_lo), plan.planes(n, w // 8, H, Wd, with_lo)
            nbytes = int(L.load().rsa_gaterv3_local_workspace_bytes(n, H, Wd, w))
            if nbytes <= 0:
                raise RuntimeError('rsa_gaterv3_local_workspace_bytes refused the grid')
            b['ws'] = torch.empty(nbytes // 4, dtype=torch.float32, device=plan.device)
            b['mid'], b['r'] = plan.f32map(n, w, H, Wd), plan.f32map(n, w, H, Wd)
            plan.keep.append(b['ws'])
        cache[key] = b
        return b

    def _gated_cnn(self, plan: Plan, blk, n, H, Wd, w, cur, bufs) -> Planes:
        """norm -> fc1 -> (token mixer ->) gate of a GatedCNNBlock on the stream ``cur``; returns the planes fc2 reads."""
        N_pl, F_pl, M_pl = bufs['norm'], bufs['fc1'], bufs['gate']
        self._rmsnorm(plan, cur, n, H, Wd, w, blk['norm'], N_pl)
        plan.conv(ops.conv_params(blk['fc1'], N_pl, H, Wd, out=F_pl))
        if blk['att']:
            self._mixer(plan, blk, n, H, Wd, w, F_pl, 2 * blk['planes'] - w // 8, bufs)  # c's planes in fc1's output: [g | i | c]
        self._gate(plan, blk, n, H, Wd, F_pl, M_pl)
        return M_pl

    def _meta_gated(self, plan: Plan, blk, n, H, Wd, w, cur, nxt, bufs, stats, W, out: Planes | None) -> None:
        N_pl, L_pl, S_pl, ws, mid, R = bufs['norm'], bufs['local'], bufs['s'], bufs['ws'], bufs['mid'], bufs['r']
        self._rmsnorm(plan, cur, n, H, Wd, w, blk['lnorm'], N_pl)
        plan.conv(ops.conv_params(blk['local1'], N_pl, H, Wd, out=L_pl))
        unit = 16 * (2 if L_pl.lo is not None else 1)
        px, pw = n * H * Wd, w // 8
        tiles = ((H + LG3.TILE_H - 1) // LG3.TILE_H) * ((Wd + LG3.TILE_W - 1) // LG3.TILE_W)
        gp = LG3.LocalGateParams()
        gp.batch, gp.H, gp.W, gp.dim, gp.fmt = n, H, Wd, w, L_pl.fmt
        L_pl.bind(gp, 'x')
        S_pl.bind(gp, 'out')
        gp.weight, gp.bias = blk['local2'][0].data_ptr(), blk['local2'][1].data_ptr()
        gp.workspace, gp.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        # byte model: the 2 w / 8 input planes read once (the halo re-reads stay on chip), s written once, one record per tile
        plan.launch('rsa_gaterv3_local_gate', gp, meta=dict(kernel='rsa_gaterv3_local_gate', flop=2 * px * (36 * 2 * w + w), bytes=px * 3 * pw * unit + n * tiles * w * 4))
        sp = LG3.ScaApplyParams()
        sp.batch, sp.H, sp.W, sp.dim, sp.fmt = n, H, Wd, w, S_pl.fmt
        S_pl.bind(sp, 's')
        sp.sca_w, sp.sca_b, sp.gamma0 = blk['sca'][0].data_ptr(), blk['sca'][1].data_ptr(), blk['gamma0'].data_ptr()
        sp.short_f32, sp.out_f32 = cur.data_ptr(), mid.data_ptr()
        sp.workspace, sp.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        plan.launch('rsa_gaterv3_sca_apply', sp, kernels=2,
                    meta=dict(kernel='rsa_gaterv3_sca_apply', flop=2 * px * w + 2 * n * w * w, bytes=px * (pw * unit + 8 * w) + n * (tiles * w + w * w) * 4))  # fmt: skip
        m = self._gated_cnn(plan, blk, n, H, Wd, w, mid, bufs)
        plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, act=L.ACT_MISH, out_f32=R))
        plan.launch('rsa_group_norm_apply', plk.group_norm_apply_params(R, w, 1, stats, blk['gamma1'], W['zeros'], mid, out, nxt))

    def _stage(self, plan: Plan, W, prefix, nb, n, H, Wd, w, cur, with_lo, cache, stats, out: Planes):
        """``nb`` MetaGated blocks on the stream ``cur`` (left intact); the last one also writes ``out`` planes.  Returns the final stream."""
        bufs = self._bufs(plan, n, H, Wd, w, False, with_lo, cache)
        a, b = plan.f32map(n, w, H, Wd), plan.f32map(n, w, H, Wd)
        for i in range(nb):
            nxt = a if cur is not a else b
            self._meta_gated(plan, W[f'{prefix}.{i}'], n, H, Wd, w, cur, nxt, bufs, stats, W, out if i == nb - 1 else None)
            cur = nxt
        return cur

    # ---------------------------------------------------------------- the U of the net: encoder, latent stage, decoder
    def _encoder(self, plan: Plan, W, prefix, n, Hp, Wp, x0, with_lo, cache, stats):
        """The encoder levels on the stream ``x0``: level j's last block writes the second half of the decoder's concatenation buffer of
        that level; Down = 3x3 convolution (f32 map) + rsa_pixel_unshuffle2.  Returns (the concatenation buffers, stream, H, W)."""
        dim = self.dim
        cats, cur, H, Wd = [], x0, Hp, Wp
        for j, nb in enumerate(self.enc_blocks):
            w = dim << j
            cat = plan.planes(n, 2 * w // 8, H, Wd, with_lo)  # [decode's upsampled output (w) | this level's skip (w)]
            cats.append(cat)
            self._stage(plan, W, f'{prefix}.{j}.gated', nb, n, H, Wd, w, cur, with_lo, cache, stats, _view(cat, w // 8, w // 8))
            t = plan.f32map(n, w // 2, H, Wd)
            nxt = plan.f32map(n, 2 * w, H // 2, Wd // 2)
            plan.conv(ops.conv_params(W[f'{prefix}.{j}.scale.0'], cat, H, Wd, in_plane0=w // 8, out_f32=t))
            plan.launch('rsa_pixel_unshuffle2', dict(x_f32=t, batch=n, H=H, W=Wd, C=w // 2, out_f32=nxt),
                        meta=dict(kernel='rsa_pixel_unshuffle2', flop=0, bytes=2 * n * H * Wd * 2 * w))  # fmt: skip
            cur, H, Wd = nxt, H // 2, Wd // 2
        return cats, cur, H, Wd

    def _latent(self, plan: Plan, W, n, H, Wd, cur, att, with_lo, cache) -> Planes:
        """The latent GatedCNNBlocks (no residual) on the stream ``cur``; returns the planes the decoder reads."""
        wl = self.dim << self.levels
        bufs = self._bufs(plan, n, H, Wd, wl, att, with_lo, cache)
        la, lb = plan.f32map(n, wl, H, Wd), plan.f32map(n, wl, H, Wd)
        prev = plan.planes(n, wl // 8, H, Wd, with_lo)
        for i in range(self.num_latent):
            blk = W[f'latent.{i}']
            m = self._gated_cnn(plan, blk, n, H, Wd, wl, cur, bufs)
            nxt = la if cur is not la else lb
            last = i == self.num_latent - 1
            plan.conv(ops.conv_params(blk['fc2'], m, H, Wd, act=L.ACT_MISH, out=prev if last else None, out_f32=None if last else nxt))
            cur = nxt
        return prev

    def _decoder(self, plan: Plan, W, n, H, Wd, prev: Planes, cats, with_lo, cache, stats, out_last: Planes | None = None):
        """The decoder levels from the latent planes ``prev``: Up = 3x3 convolution stored through depth-to-space + the layout kernel that
        writes its planes into the concatenation buffer; ``shor`` (1x1) reads the concatenation without a copy.  The last block of the last
        level also writes ``out_last`` planes where given.  Returns the final stream."""
        dim, Lv = self.dim, self.levels
        cur = None
        for i, nb in enumerate(self.dec_blocks):
            wb = dim << (Lv - i)
            w = wb // 2
            cat = cats[Lv - 1 - i]
            shuffled = torch.empty((n, w, 2 * H, 2 * Wd), dtype=torch.float32, device=plan.device)
            plan.keep.append(shuffled)
            plan.conv(ops.conv_params(W[f'decode.{i}.scale.0'], prev, H, Wd, out_nchw=shuffled, pixel_shuffle=2))
            H, Wd = 2 * H, 2 * Wd
            half = _view(cat, 0, w // 8)
            plan.call(lambda src=shuffled, dst=half: ops.nchw_to_planes(src, dst))
            plan.count_launches(1)
            sd_ = plan.f32map(n, w, H, Wd)
            plan.conv(ops.conv_params(W[f'decode.{i}.shor'], cat, H, Wd, out_f32=sd_))
            last = i == Lv - 1
            prev = out_last if last else plan.planes(n, w // 8, H, Wd, with_lo)
            cur = self._stage(plan, W, f'decode.{i}.gated', nb, n, H, Wd, w, sd_, with_lo, cache, stats, prev)
        return cur
