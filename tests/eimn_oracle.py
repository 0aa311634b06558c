"""Plain-torch EIMN: a functional restatement of ``resselt/archs/eimn/arch.py`` in EVAL mode on a state dict (cited by line), the same
forward through the engine's pack-time folds as f64 convolutions (``folded_forward``), and the f64 pieces the kernel tests compare against.

Everything runs in the dtype of ``x`` (the state dict is cast to it): fp32 for the fixtures, f64 for the fold and kernel checks.
"""

import re

import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def _conv(sd, name, x, **kw):
    return F.conv2d(x, sd[f'{name}.weight'], sd[f'{name}.bias'], **kw)


def _bn(sd, name, x):
    """nn.BatchNorm2d in eval mode (:160, :163): the running statistics."""
    return F.batch_norm(x, sd[f'{name}.running_mean'], sd[f'{name}.running_var'], sd[f'{name}.weight'], sd[f'{name}.bias'], False, 0.0, BN_EPS)


def layernorm_cf(x, weight, bias, eps=1e-6):
    """LayerNorm, channels_first (:30-34)."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return weight[:, None, None] * x + bias[:, None, None]


def dffm(sd, p, x):
    """DFFM.forward (:83-92)."""
    b = x.shape[0]
    n = layernorm_cf(x, sd[f'{p}.norm.weight'], sd[f'{p}.norm.bias'])
    x_global = F.gelu(_conv(sd, f'{p}.global_reduce', F.adaptive_avg_pool2d(n, 1)))
    x_local = F.gelu(_conv(sd, f'{p}.local_reduce', n))
    c_attn = torch.sigmoid(_conv(sd, f'{p}.channel_expand', x_global))
    s_attn = torch.sigmoid(_conv(sd, f'{p}.spatial_expand', torch.cat([x_local, x_global.expand(b, -1, x.shape[2], x.shape[3])], dim=1)))
    return x * (c_attn * s_attn)


def sadffm(sd, p, x):
    """SADFFM.forward (:56-62); Dropout is the identity."""
    x = _conv(sd, f'{p}.linear_in', x)
    x1, x2 = _conv(sd, f'{p}.SAL', x, padding=1, groups=x.shape[1]).chunk(2, dim=1)
    x = _conv(sd, f'{p}.linear_out', F.gelu(x1) * x2)
    return dffm(sd, f'{p}.DFFM', x)


def query_chain(sd, p, query):
    """region, the three groups and their concatenation (:141-145)."""
    dim = query.shape[1]
    c1, c2 = int(3 / 8 * dim), int(1 / 8 * dim)
    query = _conv(sd, f'{p}.region', query, padding=2, groups=dim)
    q1 = _conv(sd, f'{p}.spatial_1', query[:, :c1], padding=4, dilation=2, groups=c1)
    q2 = query[:, c1 : c1 + c2]
    q3 = _conv(sd, f'{p}.spatial_2', query[:, c1 + c2 :], padding=9, dilation=3, groups=dim - c1 - c2)
    return torch.cat([q1, q2, q3], dim=1)


def molrcm(sd, p, x):
    """MOLRCM.forward (:138-146); Silu is x * sigmoid(x) (:99-100)."""
    value = _conv(sd, f'{p}.proj_value.0', x)
    query = F.gelu(_conv(sd, f'{p}.proj_query.0', x))
    out = _conv(sd, f'{p}.fusion', query_chain(sd, p, query))
    out = out * torch.sigmoid(out)
    return _conv(sd, f'{p}.out', out * value)


def block(sd, p, x):
    """EIMNBlock.forward (:169-171); DropPath is the identity."""
    x = x + sd[f'{p}.layer_scale_1'][:, None, None] * molrcm(sd, f'{p}.attn', _bn(sd, f'{p}.norm1', x))
    return x + sd[f'{p}.layer_scale_2'][:, None, None] * sadffm(sd, f'{p}.mlp', _bn(sd, f'{p}.norm2', x))


def geometry(sd):
    """(num_stages, depths, dim, hidden, scale) as the loader infers them (__init__.py:65-73)."""
    stages = max(int(m.group(1)) for m in (re.search(r'block(\d+)', k) for k in sd) if m)
    depths = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('block1.'))
    dim = sd['head.0.weight'].shape[0]
    return stages, depths, dim, sd['block1.0.mlp.linear_in.weight'].shape[0] // 2, int(round((sd['tail.0.weight'].shape[0] // 3) ** 0.5))


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def eimn_forward(sd, x):
    """eimn.forward (:228-241)."""
    sd = _cast(sd, x.dtype)
    stages, depths, dim, _, scale = geometry(sd)
    x = _conv(sd, 'head.0', x, padding=1)
    identity = x
    for i in range(1, stages + 1):
        for j in range(depths):
            x = block(sd, f'block{i}.{j}', x)
        x = F.layer_norm(x.permute(0, 2, 3, 1), (dim,), sd[f'norm{i}.weight'], sd[f'norm{i}.bias'], 1e-5).permute(0, 3, 1, 2)
    return F.pixel_shuffle(_conv(sd, 'tail.0', identity + x, padding=1), scale)


# ------------------------------------------------------------------------------------------------------------------ f64 kernel references
def chain_f64(q, w1, b1, w2, b2, planes, gelu=True):
    """rsa_eimn_query_chain on [N, 8P, H, W] f64: w1 [8P, 25], w2 [8P, 49] (a 5x5 second stage in the first 25 taps), planes = (a, b, c).
    Built from F.conv2d with zero padding at BOTH stages, which is the reference's border."""
    pa, pb, pc = planes
    ca, cb = 8 * pa, 8 * (pa + pb)
    c = q.shape[1]
    q = F.gelu(q) if gelu else q
    r = F.conv2d(q, w1.reshape(c, 1, 5, 5), b1, padding=2, groups=c)
    out = [r[:, ca:cb]]
    if pa:
        out.insert(0, F.conv2d(r[:, :ca], w2[:ca, :25].reshape(ca, 1, 5, 5), b2[:ca], padding=4, dilation=2, groups=ca))
    if pc:
        out.append(F.conv2d(r[:, cb:], w2[cb:].reshape(c - cb, 1, 7, 7), b2[cb:], padding=9, dilation=3, groups=c - cb))
    return torch.cat(out, dim=1)


def sal_f64(x, w, b):
    """rsa_eimn_sal on [N, 2C, H, W] f64: w [2C, 9], b [2C]."""
    c2 = x.shape[1]
    y1, y2 = F.conv2d(x, w.reshape(c2, 1, 3, 3), b, padding=1, groups=c2).chunk(2, dim=1)
    return F.gelu(y1) * y2


def dffm_gates_f64(mean, f):
    """(c_attn [N, C], s_g [N]) from the pooled mean [N, C] of the normalised map; ``f``: wg, bg, wc, bc, ws, bs."""
    rc = f['wg'].shape[0]
    g = F.gelu(mean @ f['wg'].T + f['bg'])
    return torch.sigmoid(g @ f['wc'].T + f['bc']), g @ f['ws'][rc:] + f['bs'][0]


def dffm_apply_f64(z, x, c_attn, s_g, f, norm=None, add=None):
    """rsa_eimn_dffm_apply on [N, C, H, W] f64 with the given gates; ``norm`` = (gamma, beta, eps) of the stage LayerNorm."""
    rc = f['wl'].shape[0]
    n = layernorm_cf(z, f['gamma'], f['beta'])
    loc = F.gelu(torch.einsum('rc,nchw->nrhw', f['wl'], n) + f['bl'][None, :, None, None])
    s = torch.sigmoid(torch.einsum('r,nrhw->nhw', f['ws'][:rc], loc) + s_g[:, None, None])
    v = x + f['ls2'][None, :, None, None] * z * c_attn[:, :, None, None] * s[:, None]
    if norm is not None:
        v = F.layer_norm(v.permute(0, 2, 3, 1), (v.shape[1],), norm[0], norm[1], norm[2]).permute(0, 3, 1, 2)
    return v if add is None else v + add


# ------------------------------------------------------------------------------------------------------------------ the folded forward
def folded_forward(sd, x):
    """The forward as the engine's plan runs it, from ``archs/eimn/arch.py::fold_block``'s tensors, as plain f64 torch: BatchNorm and layer
    scale folded, the re-laid channel groups with their zero gaps, the stacked value | query convolution."""
    from resselt_amd.archs.eimn.arch import fold_block, query_layout

    x = x.double()
    sd = _cast(sd, torch.float64)
    stages, depths, dim, hidden, scale = geometry(sd)
    _, planes, _ = query_layout(dim)
    x = _conv(sd, 'head.0', x, padding=1)
    identity = x
    for i in range(1, stages + 1):
        for j in range(depths):
            f = fold_block(sd, f'block{i}.{j}', dim, hidden)
            vq = F.conv2d(x, f['vq_w'], f['vq_b'])
            c = chain_f64(vq[:, dim:], f['w1'], f['b1'], f['w2'], f['b2'], planes)
            fu = F.conv2d(c, f['fusion_w'], f['fusion_b'])
            x = x + F.conv2d(fu * torch.sigmoid(fu) * vq[:, :dim], f['out_w'], f['out_b'])
            g = sal_f64(F.conv2d(x, f['in_w'], f['in_b']), f['sal_w'], f['sal_b'])
            z = F.conv2d(g, f['lout_w'], f['lout_b'])
            mean = layernorm_cf(z, f['gamma'], f['beta']).mean(dim=(2, 3))
            c_attn, s_g = dffm_gates_f64(mean, f)
            last = j == depths - 1
            x = dffm_apply_f64(z, x, c_attn, s_g, f, norm=(sd[f'norm{i}.weight'], sd[f'norm{i}.bias'], 1e-5) if last else None,
                               add=identity if last and i == stages else None)  # fmt: skip
    return F.pixel_shuffle(_conv(sd, 'tail.0', x, padding=1), scale)
