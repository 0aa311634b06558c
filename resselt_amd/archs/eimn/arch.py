"""EIMN on the MI355X engine -- drop-in for ``resselt/archs/eimn/arch.py:174-241`` in EVAL mode.

BatchNorm uses its running statistics (eps 1e-5), Dropout and DropPath are the identity.  The reference module straight from the loader is
in training mode, where BatchNorm uses batch statistics; inference callers use ``.eval()``, and that is what this module computes.

An EIMNBlock (:149-171) is this launch list (``dim`` channels, ``pd = dim / 8`` planes):

  * ``norm1`` is folded (f64) into ``proj_value`` and ``proj_query``, which run as ONE stacked 1x1 convolution ``dim -> dim + query rows``;
    proj_query's GELU is applied by the chain kernel while it stages (the convolution's epilogue has one activation for all rows);
  * ``rsa_eimn_query_chain``: region (5x5) and, per channel group, spatial_1 (5x5 dilation 2) / identity / spatial_2 (7x7 dilation 3) in
    one launch, the intermediate map in LDS, zero outside the map;
  * ``fusion`` 1x1, ``rsa_eimn_silu_mul`` (silu(fusion) * value), and ``out`` 1x1 with ``layer_scale_1`` folded into its weights and bias:
    the residual stream is that convolution's ``res1``, and it also writes the planes ``linear_in`` reads;
  * ``norm2`` is folded into ``linear_in``; ``rsa_eimn_sal`` is GELU(dw3x3(x1) + b1) * (dw3x3(x2) + b2); ``linear_out`` writes an f32 map;
  * DFFM (:65-92): ``rsa_eimn_dffm_reduce`` (ordered partial sums of the channels-first LayerNorm), ``rsa_eimn_dffm_gates`` (one workgroup
    per image) and ``rsa_eimn_dffm_apply``: the spatial gate, ``x + layer_scale_2 * z * c_attn * s``, the stage's LayerNorm behind the last
    block of a stage, and the head's ``identity`` behind the last block of all -- the planes the tail convolution reads hold
    ``identity + x`` (:241).

A kernel works on planes of 8 channels.  Where ``3 dim / 8``, ``dim / 8`` or ``hidden`` is not a multiple of 8 (dim 48: groups 18 / 6 / 24,
hidden 127) the rows of proj_query and of linear_in are re-laid out at pack time (``query_layout`` / ``sal_layout``; as
``archs/mosr/arch.py::gate_layout``): every channel group and each half of ``SAL(...).chunk(2)`` starts on a plane boundary, the gaps are zero
rows with zero bias (GELU(0) = 0, so a gap stays 0 through the chain and the gate) and the consumers get zero input columns.

DFFM pools the whole input: under tiled ``upscale()`` and tile sharding every tile computes what the reference computes on that tile.
"""

from __future__ import annotations

import torch

from ...engine import lib as L
from ...engine import ops
from ...engine.base import EngineModule, Plan, check_fp16_range
from ...engine.paramtree import build_param_tree

BN_EPS = 1e-5
STAGE_LN_EPS = 1e-5  # nn.LayerNorm(dim) (:212)
DFFM_LN_EPS = 1e-6  # LayerNorm(channels_first) (:13-17)
MAX_RC = 32  # rsa_eimn_dffm_*: the reduced width dim / 4


# ------------------------------------------------------------------------------------------------------------------ pack-time folds (f64)
def query_layout(dim: int):
    """Padded positions of proj_query's rows: the groups (3/8, 1/8, 4/8 of dim; arch.py:107-111) each start on a plane boundary.
    Returns (perm, (planes_a, planes_b, planes_c), (c1, c2, c3))."""
    c1, c2, c3 = int(3 / 8 * dim), int(1 / 8 * dim), int(4 / 8 * dim)
    pa, pb, pc = (c1 + 7) // 8, (c2 + 7) // 8, (c3 + 7) // 8
    perm = list(range(c1)) + [8 * pa + i for i in range(c2)] + [8 * (pa + pb) + i for i in range(c3)]
    return perm, (pa, pb, pc), (c1, c2, c3)


def sal_layout(hidden: int):
    """Padded positions of linear_in's 2 * hidden rows: each half of ``chunk(2)`` starts on a plane boundary.  Returns (rows, planes per half)."""
    hp = (hidden + 7) // 8
    return list(range(hidden)) + [8 * hp + i for i in range(hidden)], hp


def bn_affine(sd, name: str):
    """(scale, shift) of an eval-mode BatchNorm in f64: y = x * scale + shift."""
    d = torch.float64
    s = sd[f'{name}.weight'].to(d) / torch.sqrt(sd[f'{name}.running_var'].to(d) + BN_EPS)
    return s, sd[f'{name}.bias'].to(d) - sd[f'{name}.running_mean'].to(d) * s


def _fold_in(w, b, scale, shift):
    """A 1x1 convolution behind y = x * scale + shift: no border, so the fold is exact."""
    w = w.to(torch.float64)
    return w * scale[None, :, None, None], b.to(torch.float64) + w.flatten(1) @ shift


def fold_block(sd, p: str, dim: int, hidden: int) -> dict:
    """Every tensor of block ``p`` the kernels read, in f64 and in the padded layouts (see the module docstring).  Plain torch: the loader
    test runs these through f64 convolutions against the oracle."""
    d = torch.float64
    dev = sd[f'{p}.layer_scale_1'].device
    z = lambda *shape: torch.zeros(shape, dtype=d, device=dev)  # noqa: E731
    perm, (pa, pb, pc), (c1, c2, c3) = query_layout(dim)
    qi = torch.tensor(perm, dtype=torch.long, device=dev)
    qrows = 8 * (pa + pb + pc)
    s1, t1 = bn_affine(sd, f'{p}.norm1')
    wv, bv = _fold_in(sd[f'{p}.attn.proj_value.0.weight'], sd[f'{p}.attn.proj_value.0.bias'], s1, t1)
    wq, bq = _fold_in(sd[f'{p}.attn.proj_query.0.weight'], sd[f'{p}.attn.proj_query.0.bias'], s1, t1)
    f = {}
    f['vq_w'], f['vq_b'] = z(dim + qrows, dim, 1, 1), z(dim + qrows)
    f['vq_w'][:dim], f['vq_b'][:dim] = wv, bv
    f['vq_w'][dim + qi], f['vq_b'][dim + qi] = wq, bq
    f['w1'], f['b1'], f['w2'], f['b2'] = z(qrows, 25), z(qrows), z(qrows, 49), z(qrows)
    f['w1'][qi], f['b1'][qi] = sd[f'{p}.attn.region.weight'].to(d).reshape(dim, 25), sd[f'{p}.attn.region.bias'].to(d)
    f['w2'][qi[:c1], :25], f['b2'][qi[:c1]] = sd[f'{p}.attn.spatial_1.weight'].to(d).reshape(c1, 25), sd[f'{p}.attn.spatial_1.bias'].to(d)
    f['w2'][qi[c1 + c2 :]], f['b2'][qi[c1 + c2 :]] = sd[f'{p}.attn.spatial_2.weight'].to(d).reshape(c3, 49), sd[f'{p}.attn.spatial_2.bias'].to(d)
    f['fusion_w'] = z(dim, qrows, 1, 1)
    f['fusion_w'][:, qi] = sd[f'{p}.attn.fusion.weight'].to(d)
    f['fusion_b'] = sd[f'{p}.attn.fusion.bias'].to(d)
    ls1 = sd[f'{p}.layer_scale_1'].to(d)
    f['out_w'], f['out_b'] = sd[f'{p}.attn.out.weight'].to(d) * ls1[:, None, None, None], sd[f'{p}.attn.out.bias'].to(d) * ls1
    rows, hp = sal_layout(hidden)
    ri = torch.tensor(rows, dtype=torch.long, device=dev)
    s2, t2 = bn_affine(sd, f'{p}.norm2')
    wi, bi = _fold_in(sd[f'{p}.mlp.linear_in.weight'], sd[f'{p}.mlp.linear_in.bias'], s2, t2)
    f['in_w'], f['in_b'] = z(16 * hp, dim, 1, 1), z(16 * hp)
    f['in_w'][ri], f['in_b'][ri] = wi, bi
    f['sal_w'], f['sal_b'] = z(16 * hp, 9), z(16 * hp)
    f['sal_w'][ri], f['sal_b'][ri] = sd[f'{p}.mlp.SAL.weight'].to(d).reshape(2 * hidden, 9), sd[f'{p}.mlp.SAL.bias'].to(d)
    f['lout_w'] = z(dim, 8 * hp, 1, 1)
    f['lout_w'][:, :hidden] = sd[f'{p}.mlp.linear_out.weight'].to(d)
    f['lout_b'] = sd[f'{p}.mlp.linear_out.bias'].to(d)
    q = f'{p}.mlp.DFFM'
    f['gamma'], f['beta'] = sd[f'{q}.norm.weight'].to(d), sd[f'{q}.norm.bias'].to(d)
    f['wg'], f['bg'] = sd[f'{q}.global_reduce.weight'].to(d).flatten(1), sd[f'{q}.global_reduce.bias'].to(d)
    f['wl'], f['bl'] = sd[f'{q}.local_reduce.weight'].to(d).flatten(1), sd[f'{q}.local_reduce.bias'].to(d)
    f['wc'], f['bc'] = sd[f'{q}.channel_expand.weight'].to(d).flatten(1), sd[f'{q}.channel_expand.bias'].to(d)
    f['ws'], f['bs'] = sd[f'{q}.spatial_expand.weight'].to(d).flatten(), sd[f'{q}.spatial_expand.bias'].to(d)
    f['ls2'] = sd[f'{p}.layer_scale_2'].to(d)
    return f


def _half_planes(w: torch.Tensor) -> torch.Tensor:
    """[channels, taps] -> [half plane][tap][4 channels] f32, the row order of rsa_eimn_query_chain."""
    c, k = w.shape
    return w.reshape(c // 4, 4, k).permute(0, 2, 1).to(torch.float32).contiguous()


class EIMN(EngineModule):
    hyperparameters = {}
    # 'auto' stays on three bf16 products: against the reference's vectors one fp16 product is off by 2.7e-3 and one bf16 product by 2.1e-2
    # where three bf16 products are off by 4.4e-5 (tests/test_eimn_gpu.py), far above the 2e-4 a cheaper 'auto' must keep
    auto_precision = 'bf16x3'
    precisions = ('bf16x3', 'bf16', 'fp16')

    def __init__(self, *, embed_dims: int = 64, scale: int = 4, depths: int = 1, hidden: int | None = None, mlp_ratios: float = 2.66,
                 num_stages: int = 16) -> None:  # fmt: skip
        super().__init__()
        dim = embed_dims
        hidden = int(dim * mlp_ratios) if hidden is None else int(hidden)
        if dim % 8 or dim < 8:
            raise NotImplementedError(f'EIMN: embed_dims must be a multiple of 8 (a plane holds 8 channels), got {dim}')
        if dim // 4 > MAX_RC:
            raise NotImplementedError(f'EIMN: embed_dims / 4 must be <= {MAX_RC} (the DFFM kernels keep the reduced vector in registers), got {dim // 4}')
        if hidden < 1:
            raise NotImplementedError(f'EIMN: the hidden width must be >= 1, got {hidden}')
        if depths < 1 or num_stages < 1:
            raise NotImplementedError(f'EIMN: depths and num_stages must be >= 1, got {depths} and {num_stages}')
        if scale < 1:
            raise NotImplementedError(f'EIMN: scale must be >= 1, got {scale}')
        self.embed_dims, self.scale, self.depths, self.hidden, self.num_stages = dim, scale, depths, hidden, num_stages
        self.mlp_ratios = hidden / dim
        rc = self.reduce_channels = int(dim * 0.25)
        _, _, (c1, _, c3) = query_layout(dim)
        s: dict = {}
        buffers: dict = {}

        def conv(name, co, ci, k):
            s[f'{name}.weight'] = (co, ci, k, k)
            s[f'{name}.bias'] = (co,)

        def bn(name):
            s[f'{name}.weight'] = (dim,)
            s[f'{name}.bias'] = (dim,)
            buffers[f'{name}.running_mean'] = torch.zeros(dim)
            buffers[f'{name}.running_var'] = torch.ones(dim)
            buffers[f'{name}.num_batches_tracked'] = torch.tensor(0, dtype=torch.long)

        conv('head.0', dim, 3, 3)
        conv('tail.0', 3 * scale * scale, dim, 3)
        for i in range(1, num_stages + 1):
            for j in range(depths):
                p = f'block{i}.{j}'
                s[f'{p}.layer_scale_1'] = (dim,)
                s[f'{p}.layer_scale_2'] = (dim,)
                bn(f'{p}.norm1')
                s[f'{p}.attn.region.weight'], s[f'{p}.attn.region.bias'] = (dim, 1, 5, 5), (dim,)
                s[f'{p}.attn.spatial_1.weight'], s[f'{p}.attn.spatial_1.bias'] = (c1, 1, 5, 5), (c1,)
                s[f'{p}.attn.spatial_2.weight'], s[f'{p}.attn.spatial_2.bias'] = (c3, 1, 7, 7), (c3,)
                conv(f'{p}.attn.fusion', dim, dim, 1)
                conv(f'{p}.attn.proj_value.0', dim, dim, 1)
                conv(f'{p}.attn.proj_query.0', dim, dim, 1)
                conv(f'{p}.attn.out', dim, dim, 1)
                bn(f'{p}.norm2')
                conv(f'{p}.mlp.linear_in', 2 * hidden, dim, 1)
                s[f'{p}.mlp.SAL.weight'], s[f'{p}.mlp.SAL.bias'] = (2 * hidden, 1, 3, 3), (2 * hidden,)
                conv(f'{p}.mlp.linear_out', dim, hidden, 1)
                q = f'{p}.mlp.DFFM'
                s[f'{q}.norm.weight'], s[f'{q}.norm.bias'] = (dim,), (dim,)
                conv(f'{q}.global_reduce', rc, dim, 1)
                conv(f'{q}.local_reduce', rc, dim, 1)
                conv(f'{q}.channel_expand', dim, rc, 1)
                conv(f'{q}.spatial_expand', 1, 2 * rc, 1)
            s[f'norm{i}.weight'], s[f'norm{i}.bias'] = (dim,), (dim,)
        build_param_tree(self, s, buffers)

    def _blocks(self):
        for i in range(1, self.num_stages + 1):
            for j in range(self.depths):
                yield i, j, f'block{i}.{j}'

    def macs_per_input_pixel(self) -> int:
        """Algorithmic multiply-accumulates per input pixel: every convolution (depthwise ones included) and DFFM's per-pixel branch (the
        local 1x1 reduction and its share of the one-channel spatial gate); the pooled branch acts on one vector per image and is not counted."""
        d, h, rc, sc = self.embed_dims, self.hidden, self.reduce_channels, self.scale
        _, _, (c1, _, c3) = query_layout(d)
        attn = 2 * d * d + 25 * d + 25 * c1 + 49 * c3 + d * d + d * d
        mlp = d * 2 * h + 9 * 2 * h + h * d + d * rc + rc
        return 27 * d + self.num_stages * self.depths * (attn + mlp) + 9 * d * 3 * sc * sc

    # ---------------------------------------------------------------- weights
    def _pack(self, device, products):
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in self.state_dict().items()}
        f32 = torch.float32
        cw = lambda w, b: ops.ConvWeights.from_oihw(w.to(f32), b.to(f32), products, device=device)  # noqa: E731
        vec = lambda t: t.to(f32).contiguous()  # noqa: E731
        W: dict = {'head': cw(sd['head.0.weight'], sd['head.0.bias']), 'tail': cw(sd['tail.0.weight'], sd['tail.0.bias'])}
        for _, _, p in self._blocks():
            f = fold_block(sd, p, self.embed_dims, self.hidden)
            W[p] = dict(
                vq=cw(f['vq_w'], f['vq_b']), fusion=cw(f['fusion_w'], f['fusion_b']), out=cw(f['out_w'], f['out_b']), lin=cw(f['in_w'], f['in_b']),
                lout=cw(f['lout_w'], f['lout_b']), w1=_half_planes(f['w1']), b1=vec(f['b1']), w2=_half_planes(f['w2']), b2=vec(f['b2']),
                sal_w=vec(f['sal_w']), sal_b=vec(f['sal_b']),
                **{k: vec(f[k]) for k in ('gamma', 'beta', 'wg', 'bg', 'wl', 'bl', 'wc', 'bc', 'ws', 'bs', 'ls2')},
            )  # fmt: skip
        for i in range(1, self.num_stages + 1):
            W[f'norm{i}'] = (sd[f'norm{i}.weight'].contiguous(), sd[f'norm{i}.bias'].contiguous())
        check_fp16_range([W['head'], W['tail']] + [v for blk in W.values() if isinstance(blk, dict) for v in blk.values()])
        return W

    # ---------------------------------------------------------------- plan
    def _build_plan(self, plan: Plan, W, x_shape, dtype, products):
        n, c, h, w = x_shape
        if c != 3:
            raise RuntimeError(f'model expects 3 input channels, got {c}')
        dim, hidden, rc = self.embed_dims, self.hidden, self.reduce_channels
        pd = dim // 8
        _, (pa, pb, pc), _ = query_layout(dim)
        qp = pa + pb + pc
        _, hp = sal_layout(hidden)
        with_lo = products == 3
        dev = plan.device
        lib = L.load()
        px = n * h * w
        unit = 16 * (2 if with_lo else 1)

        x_pl = plan.planes(n, 1, h, w, with_lo)

        def set_input(x):
            ops.nchw_to_planes(x, x_pl)

        ident, A, B, Z = (plan.f32map(n, dim, h, w) for _ in range(4))
        X_pl, X1_pl, F_pl = (plan.planes(n, pd, h, w, with_lo) for _ in range(3))
        VQ_pl = plan.planes(n, pd + qp, h, w, with_lo)
        Q_pl = plan.planes(n, qp, h, w, with_lo)
        S_pl = plan.planes(n, 2 * hp, h, w, with_lo)
        G_pl = plan.planes(n, hp, h, w, with_lo)
        ws_bytes = int(lib.rsa_eimn_dffm_workspace_bytes(n, h, w, dim))
        if ws_bytes < 0:
            raise RuntimeError(f'rsa_eimn_dffm_workspace_bytes refused {n}x{dim}x{h}x{w}')
        work = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=dev)
        gates = torch.empty((n, dim + 4), dtype=torch.float32, device=dev)
        plan.keep += [work, gates]
        geo = dict(batch=n, H=h, W=w, fmt=X_pl.fmt)
        size = dict(batch=n, H=h, W=w, C=dim)
        scratch = dict(workspace=work, workspace_bytes=ws_bytes)

        plan.conv(ops.conv_params(W['head'], x_pl, h, w, out=X_pl, out_f32=ident))
        cur = ident
        last = (self.num_stages, self.depths - 1)
        for i, j, p in self._blocks():
            blk = W[p]
            plan.conv(ops.conv_params(blk['vq'], X_pl, h, w, out=VQ_pl))
            # byte models: every operand touched once (halo re-reads stay on chip)
            plan.launch('rsa_eimn_query_chain', dict(q=(VQ_pl, pd), out=Q_pl, planes_a=pa, planes_b=pb, planes_c=pc, gelu_in=1, w1=blk['w1'], b1=blk['b1'],
                                                     w2=blk['w2'], b2=blk['b2'], **geo),
                        meta=dict(kernel='rsa_eimn_query_chain', flop=2 * px * 8 * (25 * qp + 25 * pa + 49 * pc), bytes=px * qp * unit * 2))  # fmt: skip
            plan.conv(ops.conv_params(blk['fusion'], Q_pl, h, w, out=F_pl))
            plan.launch('rsa_eimn_silu_mul', dict(f=F_pl, v=VQ_pl, out=F_pl, planes=pd, **geo),
                        meta=dict(kernel='rsa_eimn_silu_mul', flop=px * dim * 2, bytes=px * pd * unit * 3))  # fmt: skip
            plan.conv(ops.conv_params(blk['out'], F_pl, h, w, res1=cur, alpha=1.0, out_f32=A, out=X1_pl))
            plan.conv(ops.conv_params(blk['lin'], X1_pl, h, w, out=S_pl))
            plan.launch('rsa_eimn_sal', dict(in_=S_pl, out=G_pl, planes=hp, weight=blk['sal_w'], bias=blk['sal_b'], **geo),
                        meta=dict(kernel='rsa_eimn_sal', flop=2 * px * 16 * hp * 9, bytes=px * hp * unit * 3))  # fmt: skip
            plan.conv(ops.conv_params(blk['lout'], G_pl, h, w, out_f32=Z))
            ng, nb = W[f'norm{i}'] if j == self.depths - 1 else (None, None)
            add = ident if (i, j) == last else None
            ln = dict(gamma=blk['gamma'], beta=blk['beta'], eps=DFFM_LN_EPS)
            dffm = (
                ('rsa_eimn_dffm_reduce', dict(z=Z, **size, **ln, **scratch)),
                ('rsa_eimn_dffm_gates', dict(**scratch, **size, rc=rc, wg=blk['wg'], bg=blk['bg'], wc=blk['wc'], bc=blk['bc'], ws=blk['ws'], bs=blk['bs'], gates=gates)),
                ('rsa_eimn_dffm_apply', dict(z=Z, x=A, rc=rc, **ln, wl=blk['wl'], bl=blk['bl'], ws=blk['ws'], gates=gates, scale=blk['ls2'], norm_gamma=ng,
                                             norm_beta=nb, norm_eps=STAGE_LN_EPS, add=add, out_f32=B, out=X_pl, C=dim, **geo)),
            )  # fmt: skip
            # z read by both passes, x read, the stream and the planes written (+ the added map)
            plan.launch(dffm, kernels=3,
                        meta=dict(kernel='rsa_eimn_dffm', flop=2 * px * dim * (rc + 8), bytes=px * dim * 4 * (4 + (add is not None)) + px * pd * unit))  # fmt: skip
            cur = B
        s = self.scale
        y = plan.output((n, 3, h * s, w * s), dtype)
        plan.conv(ops.conv_params(W['tail'], X_pl, h, w, out_nchw=y, pixel_shuffle=s))
        return set_input
