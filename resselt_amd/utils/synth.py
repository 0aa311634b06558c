"""Deterministic synthetic checkpoints (there is no network: no real weights can be downloaded).

Every tensor is drawn from uniform(-1/sqrt(fan_in), +1/sqrt(fan_in)) -- PyTorch's default conv/linear
init scale -- by a numpy PCG64 stream keyed by the tensor's *name*, so the same state dict can be rebuilt
bit-for-bit on the GPU box without the reference, and the golden fixtures in ``tests/golden`` only need to
store seeds, inputs and expected outputs.
"""

from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np
import torch

from ..engine.paramtree import ParamShapes
from ..engine.transformer import tail_shapes


def synth_tensor(name: str, shape, fan_in: int, seed: int = 0, scale: float = 1.0) -> torch.Tensor:
    rng = np.random.Generator(np.random.PCG64([zlib.crc32(name.encode()), seed]))
    bound = scale / float(np.sqrt(max(fan_in, 1)))
    a = rng.uniform(-bound, bound, size=tuple(shape)).astype(np.float32)
    return torch.from_numpy(a)


def synth_input(shape, seed: int = 0) -> torch.Tensor:
    """Image-like input in [0, 1), fp32."""
    rng = np.random.Generator(np.random.PCG64([0x1A6E, seed]))
    return torch.from_numpy(rng.random(size=tuple(shape), dtype=np.float32))


def _conv(sd, name, cout, cin, k, seed, bias=True, scale=1.0):
    fan_in = cin * k * k
    sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (cout, cin, k, k), fan_in, seed, scale)
    if bias:
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (cout,), fan_in, seed, scale)


def _resi_conv(sd, name, C, resi, seed):
    """The 1conv / 3conv tail of a residual group, from the shapes the models register (engine/transformer.py: ``tail_shapes``)."""
    shapes = ParamShapes()
    tail_shapes(shapes, name, C, resi)
    for key, (cout, cin, k, _) in ((key, shape) for key, shape in shapes.items() if key.endswith('.weight')):
        _conv(sd, key[: -len('.weight')], cout, cin, k, seed)


def rrdbnet_state_dict(in_nc=3, out_nc=3, nf=64, nb=23, gc=32, scale=4, plus=False, seed=0, new_arch=False) -> 'OrderedDict[str, torch.Tensor]':
    """Old-arch (ESRGAN) keys; ``new_arch=True`` renames them to the official Real-ESRGAN spelling."""
    sd: OrderedDict = OrderedDict()
    _conv(sd, 'model.0', nf, in_nc, 3, seed)
    for i in range(nb):
        for r in (1, 2, 3):
            p = f'model.1.sub.{i}.RDB{r}'
            if plus:
                _conv(sd, f'{p}.conv1x1', gc, nf, 1, seed, bias=False)
            for j in range(1, 6):
                _conv(sd, f'{p}.conv{j}.0', gc if j < 5 else nf, nf + (j - 1) * gc, 3, seed)
    _conv(sd, f'model.1.sub.{nb}', nf, nf, 3, seed)
    k = 3
    n_up = {1: 0, 2: 1, 4: 2, 8: 3}[scale]
    for _ in range(n_up):
        _conv(sd, f'model.{k}', nf, nf, 3, seed)
        k += 3
    k -= 1
    _conv(sd, f'model.{k}', nf, nf, 3, seed)
    _conv(sd, f'model.{k + 2}', out_nc, nf, 3, seed)
    if not new_arch:
        return sd
    out: OrderedDict = OrderedDict()
    for key, v in sd.items():
        parts = key.split('.')
        kind = parts[-1]
        if key.startswith('model.0.'):
            out[f'conv_first.{kind}'] = v
        elif key.startswith('model.1.sub.') and len(parts) == 5:
            out[f'conv_body.{kind}'] = v
        elif key.startswith('model.1.sub.'):
            out[f'body.{parts[3]}.rdb{parts[4][3:]}.{parts[5]}.{kind}'] = v
        else:
            idx = int(parts[1])
            if idx == k:
                out[f'conv_hr.{kind}'] = v
            elif idx == k + 2:
                out[f'conv_last.{kind}'] = v
            else:
                out[f'conv_up{idx // 3}.{kind}'] = v
    return out


def rrdbnet_heavy_tailed_state_dict(nb=23, nf=64, gc=32, seed=0, df=3.0, outlier_gain=32.0, outlier_every=5) -> 'OrderedDict[str, torch.Tensor]':
    """RRDBNet checkpoint with the statistics uniform synthetic weights lack: heavy-tailed weights and outlier activation channels.

    * every weight tensor is re-drawn from a Student-t (``df`` degrees of freedom) scaled to the variance of the default uniform
      init, so single weights reach 10-30x the typical magnitude;
    * inside every RDB, every ``outlier_every``-th growth channel of x1..x4 is scaled by ``outlier_gain`` at its producer (weight row
      and bias) and by ``1 / outlier_gain`` at every consumer (weight column).  LeakyReLU is positively homogeneous, so the network
      function is unchanged, but those channels carry activations ``outlier_gain`` times larger than their neighbours -- the
      situation in which a hi/lo operand split and an f32 accumulator are stressed.
    """
    sd = rrdbnet_state_dict(nf=nf, nb=nb, gc=gc, seed=seed)
    for name in list(sd):
        t = sd[name]
        fan_in = t[0].numel() if name.endswith('.weight') else sd[name[: -len('bias')] + 'weight'][0].numel()
        rng = np.random.Generator(np.random.PCG64([zlib.crc32(name.encode()), seed, 0x7A11]))
        a = rng.standard_t(df, size=tuple(t.shape)).astype(np.float32)
        a *= float(np.sqrt(1.0 / (3.0 * fan_in)) / np.sqrt(df / (df - 2.0)))  # variance of uniform(+-1/sqrt(fan_in)) = 1 / (3 fan_in)
        sd[name] = torch.from_numpy(a)
    g = float(outlier_gain)
    for i in range(nb):
        for r in (1, 2, 3):
            p = f'model.1.sub.{i}.RDB{r}'
            for j in range(1, 5):
                chans = list(range((i + r + j) % outlier_every, gc, outlier_every))
                sd[f'{p}.conv{j}.0.weight'][chans] *= g
                sd[f'{p}.conv{j}.0.bias'][chans] *= g
                cols = [nf + (j - 1) * gc + c for c in chans]
                for m in range(j + 1, 6):
                    sd[f'{p}.conv{m}.0.weight'][:, cols] /= g
    return sd


def _conv3xc(sd, name, cout, cin, gain, seed):
    _conv(sd, f'{name}.sk', cout, cin, 1, seed)
    _conv(sd, f'{name}.conv.0', cin * gain, cin, 1, seed)
    _conv(sd, f'{name}.conv.1', cout * gain, cin * gain, 3, seed)
    _conv(sd, f'{name}.conv.2', cout, cout * gain, 1, seed)
    # stored eval_conv is overwritten by the fold on every reference forward; keep a placeholder of the right shape
    _conv(sd, f'{name}.eval_conv', cout, cin, 3, seed)


def _spab(sd, name, c, seed):
    for r in ('c1_r', 'c2_r', 'c3_r'):
        _conv3xc(sd, f'{name}.{r}', c, c, 2, seed)


def spanplus_state_dict(num_in_ch=3, num_out_ch=3, blocks=(4,), feature_channels=48, upscale=4, upsampler='ps', seed=0):
    sd: OrderedDict = OrderedDict()
    fc = feature_channels
    _conv3xc(sd, 'feats.0', fc, num_in_ch, 2, seed)
    for bi, nblk in enumerate(blocks):
        p = f'feats.{bi + 1}'
        _spab(sd, f'{p}.block_1', fc, seed)
        for j in range(nblk):
            _spab(sd, f'{p}.block_n.{j}', fc, seed)
        _spab(sd, f'{p}.block_end', fc, seed)
        _conv3xc(sd, f'{p}.conv_2', fc, fc, 2, seed)
        _conv(sd, f'{p}.conv_cat', fc, fc * 4, 1, seed)
    if upsampler == 'ps':
        _conv(sd, 'upsampler.0', num_in_ch * upscale * upscale, fc, 3, seed)
    else:
        groups = 4
        oc = 2 * groups * upscale * upscale
        _conv(sd, 'upsampler.end_conv', num_out_ch, fc, 1, seed)
        _conv(sd, 'upsampler.offset', oc, fc, 1, seed)
        _conv(sd, 'upsampler.scope', oc, fc, 1, seed, bias=False)
        h = torch.arange((-upscale + 1) / 2, (upscale - 1) / 2 + 1) / upscale
        sd['upsampler.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, groups, 1).reshape(1, -1, 1, 1)
    return sd


def span_state_dict(num_in_ch=3, feature_channels=48, upscale=4, seed=0, norm=True):
    sd: OrderedDict = OrderedDict()
    fc = feature_channels
    _conv3xc(sd, 'conv_1', fc, num_in_ch, 2, seed)
    for i in range(1, 7):
        _spab(sd, f'block_{i}', fc, seed)
    _conv(sd, 'conv_cat', fc, fc * 4, 1, seed)
    _conv3xc(sd, 'conv_2', fc, fc, 2, seed)
    _conv(sd, 'upsampler.0', num_in_ch * upscale * upscale, fc, 3, seed)
    if not norm:
        sd['no_norm'] = torch.zeros(1)
    return sd


def swinir_state_dict(in_ch=3, embed_dim=60, depths=(2, 2), num_heads=(6, 6), window=8, mlp_ratio=2.0, upscale=2, upsampler='nearest+conv',
                      resi='1conv', img_size=64, seed=0, scale=1.0):
    """Keys of the reference SwinIR module (archs/swinir/arch.py:735-960) incl. its registered buffers.

    LayerNorm weights are 1 + u, biases and the relative-position table are drawn at the same +-1/sqrt(fan_in) scale.
    """
    sd: OrderedDict = OrderedDict()
    C = embed_dim
    hidden = int(C * mlp_ratio)

    def lin(name, cout, cin, bias=True):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (cout, cin), cin, seed, scale)
        if bias:
            sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (cout,), cin, seed, scale)

    def ln(name):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (C,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (C,), 16, seed)

    # relative_position_index buffer (arch.py:111-122)
    ch, cw = torch.arange(window), torch.arange(window)
    coords = torch.stack(torch.meshgrid([ch, cw], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    rp_index = rel.sum(-1)

    def shift_mask():
        H = W = img_size
        s_ = window // 2
        img = torch.zeros(1, H, W, 1)
        cnt = 0
        for hs in (slice(0, -window), slice(-window, -s_), slice(-s_, None)):
            for ws in (slice(0, -window), slice(-window, -s_), slice(-s_, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
        mw = img.view(1, H // window, window, W // window, window, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, window * window)
        d = mw.unsqueeze(1) - mw.unsqueeze(2)
        return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))

    _conv(sd, 'conv_first', C, in_ch, 3, seed)
    ln('patch_embed.norm')
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f'layers.{i}.residual_group.blocks.{j}'
            if j % 2 == 1:
                sd[f'{b}.attn_mask'] = shift_mask()
            ln(f'{b}.norm1')
            sd[f'{b}.attn.relative_position_bias_table'] = synth_tensor(f'{b}.rpb', ((2 * window - 1) ** 2, num_heads[i]), 4, seed)
            sd[f'{b}.attn.relative_position_index'] = rp_index.clone()
            lin(f'{b}.attn.qkv', 3 * C, C)
            lin(f'{b}.attn.proj', C, C)
            ln(f'{b}.norm2')
            lin(f'{b}.mlp.fc1', hidden, C)
            lin(f'{b}.mlp.fc2', C, hidden)
        _resi_conv(sd, f'layers.{i}.conv', C, resi, seed)
    ln('norm')
    _resi_conv(sd, 'conv_after_body', C, resi, seed)
    nf = 64
    if upsampler == 'nearest+conv':
        _conv(sd, 'conv_before_upsample.0', nf, C, 3, seed)
        for u in range(1, {2: 1, 4: 2, 8: 3}[upscale] + 1):
            _conv(sd, f'conv_up{u}', nf, nf, 3, seed)
        _conv(sd, 'conv_hr', nf, nf, 3, seed)
        _conv(sd, 'conv_last', in_ch, nf, 3, seed)
    elif upsampler == 'pixelshuffle':
        _conv(sd, 'conv_before_upsample.0', nf, C, 3, seed)
        if upscale == 3:
            _conv(sd, 'upsample.0', 9 * nf, nf, 3, seed)
        else:
            for u in range({2: 1, 4: 2, 8: 3}[upscale]):
                _conv(sd, f'upsample.{2 * u}', 4 * nf, nf, 3, seed)
        _conv(sd, 'conv_last', in_ch, nf, 3, seed)
    elif upsampler == 'pixelshuffledirect':
        _conv(sd, 'upsample.0', upscale * upscale * in_ch, C, 3, seed)
    else:
        _conv(sd, 'conv_last', in_ch, C, 3, seed)
    return sd


def compact_state_dict(num_in_ch=3, num_feat=64, num_conv=16, upscale=4, seed=0):
    """Keys of SRVGGNetCompact (archs/compact/arch.py:36-57): body.{2i} convs, body.{2i+1} PReLU slopes, last conv."""
    sd: OrderedDict = OrderedDict()
    cin = num_in_ch
    for i in range(num_conv + 1):
        _conv(sd, f'body.{2 * i}', num_feat, cin, 3, seed)
        sd[f'body.{2 * i + 1}.weight'] = 0.25 + synth_tensor(f'body.{2 * i + 1}.weight', (num_feat,), 16, seed)  # slopes in (0, 0.5)
        cin = num_feat
    _conv(sd, f'body.{2 * (num_conv + 1)}', num_in_ch * upscale * upscale, num_feat, 3, seed)
    return sd


def dat_geometry(split_size, idx: int):
    """(H_sp, W_sp) of attention branch ``idx`` (archs/dat/arch.py:186-191): branch 1 swaps the rectangle."""
    return (split_size[0], split_size[1]) if idx == 0 else (split_size[1], split_size[0])


def dat_shifted(rg_idx: int, b_idx: int) -> bool:
    """Which DATB blocks shift their windows (archs/dat/arch.py:312, 453)."""
    return (rg_idx % 2 == 0 and b_idx > 0 and (b_idx - 2) % 4 == 0) or (rg_idx % 2 != 0 and b_idx % 4 == 0)


def dat_shift_masks(H: int, W: int, split_size, shift_size):
    """The two additive shift masks [nW, N, N] (archs/dat/arch.py:336-411), one per branch."""
    out = []
    for idx in (0, 1):
        hs, ws = dat_geometry(split_size, idx)
        sh, sw = dat_geometry(shift_size, idx)
        img = torch.zeros(H, W)
        cnt = 0
        for hsl in (slice(0, -hs), slice(-hs, -sh), slice(-sh, None)):
            for wsl in (slice(0, -ws), slice(-ws, -sw), slice(-sw, None)):
                img[hsl, wsl] = cnt
                cnt += 1
        mw = img.view(H // hs, hs, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, hs * ws)
        d = mw.unsqueeze(1) - mw.unsqueeze(2)
        out.append(torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d)))
    return out


def dat_state_dict(in_chans=3, embed_dim=64, split_size=(2, 4), depth=(2,), num_heads=(4,), expansion_factor=2.0, qkv_bias=True, upscale=2,
                   resi='1conv', upsampler='pixelshuffle', img_size=16, seed=0):  # fmt: skip
    """Keys (parameters AND buffers) of the reference DAT module (archs/dat/arch.py:828-990).

    BatchNorm running statistics are synthetic too (mean ~ u, var in (0.5, 1.5)): the engine implements the eval-mode network.
    """
    sd: OrderedDict = OrderedDict()
    C = embed_dim
    hidden = int(C * expansion_factor)
    split_size = list(split_size)
    shift_size = [split_size[0] // 2, split_size[1] // 2]

    def lin(name, cout, cin, bias=True):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (cout, cin), cin, seed)
        if bias:
            sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (cout,), cin, seed)

    def ln(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), 16, seed)

    def bn(name, c):
        ln(name, c)
        sd[f'{name}.running_mean'] = synth_tensor(f'{name}.running_mean', (c,), 16, seed)
        sd[f'{name}.running_var'] = 1.0 + 2.0 * synth_tensor(f'{name}.running_var', (c,), 16, seed)
        sd[f'{name}.num_batches_tracked'] = torch.tensor(100, dtype=torch.int64)

    def dw(name, c):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (c, 1, 3, 3), 9, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), 9, seed)

    def aim(name):
        dw(f'{name}.dwconv.0', C)
        bn(f'{name}.dwconv.1', C)
        _conv(sd, f'{name}.channel_interaction.1', C // 8, C, 1, seed)
        bn(f'{name}.channel_interaction.2', C // 8)
        _conv(sd, f'{name}.channel_interaction.4', C, C // 8, 1, seed)
        _conv(sd, f'{name}.spatial_interaction.0', C // 16, C, 1, seed)
        bn(f'{name}.spatial_interaction.1', C // 16)
        _conv(sd, f'{name}.spatial_interaction.3', 1, C // 16, 1, seed)

    def spatial_branch(name, idx, heads):
        hs, ws = dat_geometry(split_size, idx)
        bh, bw = torch.arange(1 - hs, hs), torch.arange(1 - ws, ws)
        sd[f'{name}.rpe_biases'] = torch.stack(torch.meshgrid([bh, bw], indexing='ij')).flatten(1).transpose(0, 1).contiguous().float()
        coords = torch.stack(torch.meshgrid([torch.arange(hs), torch.arange(ws)], indexing='ij')).flatten(1)
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += hs - 1
        rel[:, :, 1] += ws - 1
        rel[:, :, 0] *= 2 * ws - 1
        sd[f'{name}.relative_position_index'] = rel.sum(-1)
        pos_dim = ((C // 2) // 4) // 4  # DynamicPosBias(dim // 4): pos_dim = dim // 4 again (arch.py:116, 194)
        lin(f'{name}.pos.pos_proj', pos_dim, 2)
        for k, cout in (('pos1', pos_dim), ('pos2', pos_dim), ('pos3', heads)):
            sd[f'{name}.pos.{k}.0.weight'] = 1.0 + synth_tensor(f'{name}.pos.{k}.0.weight', (pos_dim,), 16, seed)
            sd[f'{name}.pos.{k}.0.bias'] = synth_tensor(f'{name}.pos.{k}.0.bias', (pos_dim,), 16, seed)
            lin(f'{name}.pos.{k}.2', cout, pos_dim)

    _conv(sd, 'conv_first', C, in_chans, 3, seed)
    ln('before_RG.1', C)
    for i, d in enumerate(depth):
        heads = num_heads[i]
        for j in range(d):
            b = f'layers.{i}.blocks.{j}'
            ln(f'{b}.norm1', C)
            if j % 2 == 0:  # DSTB: adaptive spatial attention
                lin(f'{b}.attn.qkv', 3 * C, C, qkv_bias)
                lin(f'{b}.attn.proj', C, C)
                for idx in (0, 1):
                    spatial_branch(f'{b}.attn.attns.{idx}', idx, heads // 2)
                if dat_shifted(i, j):
                    m0, m1 = dat_shift_masks(img_size, img_size, split_size, shift_size)
                    sd[f'{b}.attn.attn_mask_0'] = m0
                    sd[f'{b}.attn.attn_mask_1'] = m1
            else:  # DCTB: adaptive channel attention
                sd[f'{b}.attn.temperature'] = 1.0 + synth_tensor(f'{b}.attn.temperature', (heads, 1, 1), 4, seed)
                lin(f'{b}.attn.qkv', 3 * C, C, qkv_bias)
                lin(f'{b}.attn.proj', C, C)
            aim(f'{b}.attn')
            lin(f'{b}.ffn.fc1', hidden, C)
            ln(f'{b}.ffn.sg.norm', hidden // 2)
            dw(f'{b}.ffn.sg.conv', hidden // 2)
            lin(f'{b}.ffn.fc2', C, hidden // 2)
            ln(f'{b}.norm2', C)
        _resi_conv(sd, f'layers.{i}.conv', C, resi, seed)
    ln('norm', C)
    _resi_conv(sd, 'conv_after_body', C, resi, seed)
    if upsampler == 'pixelshuffle':
        _conv(sd, 'conv_before_upsample.0', 64, C, 3, seed)
        if upscale == 3:
            _conv(sd, 'upsample.0', 9 * 64, 64, 3, seed)
        else:
            for u in range({1: 0, 2: 1, 4: 2, 8: 3}[upscale]):
                _conv(sd, f'upsample.{2 * u}', 4 * 64, 64, 3, seed)
        _conv(sd, 'conv_last', in_chans, 64, 3, seed)
    else:
        _conv(sd, 'upsample.0', upscale * upscale * in_chans, C, 3, seed)
    return sd


def _repconv(sd, name, cout, cin, seed):
    """Keys of SpanPP's RepConv (archs/spanpp/arch.py:152-192): SeqConv3x3 (k0, b0, k1, b1), a plain 3x3, a Conv3XC, the fused conv, alpha."""
    mid = 2 * cout
    sd[f'{name}.alpha'] = 1.0 + synth_tensor(f'{name}.alpha', (3,), 4, seed)
    sd[f'{name}.conv1.k0'] = synth_tensor(f'{name}.conv1.k0', (mid, cin, 1, 1), cin, seed)
    sd[f'{name}.conv1.b0'] = synth_tensor(f'{name}.conv1.b0', (mid,), cin, seed)
    sd[f'{name}.conv1.k1'] = synth_tensor(f'{name}.conv1.k1', (cout, mid, 3, 3), mid * 9, seed)
    sd[f'{name}.conv1.b1'] = synth_tensor(f'{name}.conv1.b1', (cout,), mid * 9, seed)
    _conv(sd, f'{name}.conv2', cout, cin, 3, seed)
    _conv3xc(sd, f'{name}.conv3', cout, cin, 2, seed)
    _conv(sd, f'{name}.conv_3x3_rep', cout, cin, 3, seed)


def spanpp_state_dict(num_in_ch=3, feature_channels=48, scale_list=(1, 2, 3, 4), implicit_dim=256, latent_layers=4, seed=0):
    """Keys of the reference SpanPP module (archs/spanpp/arch.py:315-373), ``MetaIGConv`` buffer included."""
    sd: OrderedDict = OrderedDict()
    fc = feature_channels
    _repconv(sd, 'conv0', fc, num_in_ch, seed)
    for i in range(1, 7):
        for r in ('c1_r', 'c2_r', 'c3_r'):
            _repconv(sd, f'block_{i}.{r}', fc, fc, seed)
    _conv(sd, 'conv_cat', fc, 4 * fc, 1, seed)
    _repconv(sd, 'conv_2', fc, fc, seed)
    # freq / amplitude are randn * 0.02 in the reference; a larger spread makes the generated kernels non-trivial
    sd['upsampler.freq'] = synth_tensor('upsampler.freq', (fc * 9, implicit_dim, 1, 1), 1, seed, 0.5)
    sd['upsampler.amplitude'] = synth_tensor('upsampler.amplitude', (fc * 9, implicit_dim, 1, 1), 1, seed, 0.5)
    _conv(sd, 'upsampler.phase', implicit_dim // 2, 1, 1, seed)
    for l in range(latent_layers):
        _conv(sd, f'upsampler.query_kernel.{2 * l}', implicit_dim, implicit_dim, 1, seed)
    _conv(sd, f'upsampler.query_kernel.{2 * latent_layers}', 3, implicit_dim, 1, seed)
    sd['MetaIGConv'] = torch.tensor(sorted(set(scale_list)), dtype=torch.uint8)
    return sd


def hat_rpi(window: int, overlap_ratio: float):
    """The two registered index buffers of HAT (archs/hat/arch.py:987-1034): self-attention and overlapping cross-attention."""
    co = torch.stack(torch.meshgrid([torch.arange(window), torch.arange(window)], indexing='ij')).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    sa = rel.sum(-1)
    ext = window + int(overlap_ratio * window)
    ce = torch.stack(torch.meshgrid([torch.arange(ext), torch.arange(ext)], indexing='ij')).flatten(1)
    rel = (ce[:, None, :] - co[:, :, None]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - ext + 1
    rel[:, :, 1] += window - ext + 1
    rel[:, :, 0] *= window + ext - 1
    return sa, rel.sum(-1)


def hat_state_dict(in_chans=3, embed_dim=60, depths=(2, 2), num_heads=(6, 6), window=8, compress_ratio=3, squeeze_factor=30, overlap_ratio=0.5,
                   mlp_ratio=2.0, upscale=2, num_feat=64, resi='1conv', seed=0):  # fmt: skip
    """Keys of the reference HAT module (archs/hat/arch.py:798-1110) incl. its two index buffers."""
    sd: OrderedDict = OrderedDict()
    C = embed_dim
    hidden = int(C * mlp_ratio)
    ext = window + int(overlap_ratio * window)

    def lin(name, cout, cin):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (cout, cin), cin, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (cout,), cin, seed)

    def ln(name):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (C,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (C,), 16, seed)

    sd['relative_position_index_SA'], sd['relative_position_index_OCA'] = hat_rpi(window, overlap_ratio)
    _conv(sd, 'conv_first', C, in_chans, 3, seed)
    ln('patch_embed.norm')
    for i, depth in enumerate(depths):
        g = f'layers.{i}.residual_group'
        for j in range(depth):
            b = f'{g}.blocks.{j}'
            ln(f'{b}.norm1')
            sd[f'{b}.attn.relative_position_bias_table'] = synth_tensor(f'{b}.rpb', ((2 * window - 1) ** 2, num_heads[i]), 4, seed)
            lin(f'{b}.attn.qkv', 3 * C, C)
            lin(f'{b}.attn.proj', C, C)
            _conv(sd, f'{b}.conv_block.cab.0', C // compress_ratio, C, 3, seed)
            _conv(sd, f'{b}.conv_block.cab.2', C, C // compress_ratio, 3, seed)
            _conv(sd, f'{b}.conv_block.cab.3.attention.1', C // squeeze_factor, C, 1, seed)
            _conv(sd, f'{b}.conv_block.cab.3.attention.3', C, C // squeeze_factor, 1, seed)
            ln(f'{b}.norm2')
            lin(f'{b}.mlp.fc1', hidden, C)
            lin(f'{b}.mlp.fc2', C, hidden)
        o = f'{g}.overlap_attn'
        ln(f'{o}.norm1')
        lin(f'{o}.qkv', 3 * C, C)
        sd[f'{o}.relative_position_bias_table'] = synth_tensor(f'{o}.rpb', ((window + ext - 1) ** 2, num_heads[i]), 4, seed)
        lin(f'{o}.proj', C, C)
        ln(f'{o}.norm2')
        lin(f'{o}.mlp.fc1', hidden, C)
        lin(f'{o}.mlp.fc2', C, hidden)
        if resi == '1conv':
            _conv(sd, f'layers.{i}.conv', C, C, 3, seed)
    ln('norm')
    if resi == '1conv':
        _conv(sd, 'conv_after_body', C, C, 3, seed)
    _conv(sd, 'conv_before_upsample.0', num_feat, C, 3, seed)
    if upscale == 3:
        _conv(sd, 'upsample.0', 9 * num_feat, num_feat, 3, seed)
    else:
        for u in range({1: 0, 2: 1, 4: 2, 8: 3}[upscale]):
            _conv(sd, f'upsample.{2 * u}', 4 * num_feat, num_feat, 3, seed)
    _conv(sd, 'conv_last', in_chans, num_feat, 3, seed)
    return sd


def rtmosr_state_dict(scale=2, dim=32, ffn_expansion=2.0, n_blocks=2, unshuffle_mod=False, dccm=True, se=True, seed=0):
    """Keys of the reference RTMoSR module (archs/rtmosr/arch.py:340-387)."""
    sd: OrderedDict = OrderedDict()
    unshuffle = 0
    s_int = scale
    if scale < 4 and unshuffle_mod:
        unshuffle = 4 // scale
        s_int = 4
    hidden = int(ffn_expansion * dim)
    if unshuffle:
        _repconv(sd, 'to_feat.1', dim, 3 * unshuffle * unshuffle, seed)
    else:
        _repconv(sd, 'to_feat', dim, 3, seed)
    for i in range(n_blocks):
        b = f'body.{i}'
        sd[f'{b}.norm.scale'] = 1.0 + synth_tensor(f'{b}.norm.scale', (dim,), 16, seed)
        sd[f'{b}.norm.offset'] = synth_tensor(f'{b}.norm.offset', (dim,), 16, seed)
        _repconv(sd, f'{b}.fc1', 2 * hidden, dim, seed)
        _repconv(sd, f'{b}.conv.0.poll.1', 4 * dim, dim, seed)
        o = f'{b}.conv.1'
        for k in (1, 2, 3, 4):
            sd[f'{o}.alpha{k}'] = 1.0 + synth_tensor(f'{o}.alpha{k}', (1, 4 * dim, 1, 1), 16, seed)
        for name, ks in (('conv1x1', 1), ('conv3x3', 3), ('conv5x5', 5), ('conv5x5_reparam', 5)):
            sd[f'{o}.{name}.weight'] = synth_tensor(f'{o}.{name}.weight', (4 * dim, 1, ks, ks), ks * ks, seed)
            sd[f'{o}.{name}.bias'] = synth_tensor(f'{o}.{name}.bias', (4 * dim,), ks * ks, seed)
        if se:
            _conv(sd, f'{b}.conv.2.squeezing.0', 2 * dim, 4 * dim, 1, seed)
            _conv(sd, f'{b}.conv.2.squeezing.2', 4 * dim, 2 * dim, 1, seed)
        if dccm:
            _repconv(sd, f'{b}.fc2', dim, hidden, seed)
        else:
            _conv(sd, f'{b}.fc2', dim, hidden, 1, seed)
    _repconv(sd, 'to_img.0', 3 * s_int * s_int, dim, seed)
    return sd


def drct_block_dims(embed_dim: int, gc: int, num_heads: int):
    """(dim, heads, mlp_ratio scale, shifted) of the five Swin blocks of a DRCT dense group (reference archs/drct/arch.py:225-298)."""
    out = []
    for j in range(5):
        dim = embed_dim + j * gc
        heads = num_heads if j == 0 else num_heads - (dim % num_heads)
        out.append((dim, heads, j in (1, 3)))
    return out


def drct_state_dict(in_chans=3, embed_dim=180, num_layers=2, num_heads=6, window=16, mlp_ratio=2.0, gc=32, upscale=2, resi='1conv', img_size=64,
                    seed=0, attn_mask=True):  # fmt: skip
    """Keys of the reference DRCT module (archs/drct/arch.py:617-792) incl. its registered buffers (relative_position_index, attn_mask of
    the shifted blocks swin2 / swin4).  The loader fixes depths = (6,) * num_layers and reads one head count per layer."""
    sd: OrderedDict = OrderedDict()
    C = embed_dim

    def lin(name, cout, cin):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (cout, cin), cin, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (cout,), cin, seed)

    def ln(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), 16, seed)

    coords = torch.stack(torch.meshgrid([torch.arange(window), torch.arange(window)], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    rp_index = rel.sum(-1)

    def shift_mask():
        s_ = window // 2
        img = torch.zeros(1, img_size, img_size, 1)
        cnt = 0
        for hs in (slice(0, -window), slice(-window, -s_), slice(-s_, None)):
            for ws in (slice(0, -window), slice(-window, -s_), slice(-s_, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
        mw = img.view(1, img_size // window, window, img_size // window, window, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, window * window)
        d = mw.unsqueeze(1) - mw.unsqueeze(2)
        return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))

    _conv(sd, 'conv_first', C, in_chans, 3, seed)
    ln('patch_embed.norm', C)
    for i in range(num_layers):
        for j, (dim, heads, shifted) in enumerate(drct_block_dims(C, gc, num_heads), start=1):
            b = f'layers.{i}.swin{j}'
            hidden = int(dim * (mlp_ratio if j <= 3 else 1))
            if shifted and attn_mask:  # (a checkpoint saved without the mask buffers loads as img_size = window: no block is shifted)
                sd[f'{b}.attn_mask'] = shift_mask()
            ln(f'{b}.norm1', dim)
            sd[f'{b}.attn.relative_position_bias_table'] = synth_tensor(f'{b}.attn.relative_position_bias_table', ((2 * window - 1) ** 2, heads), 16, seed)
            sd[f'{b}.attn.relative_position_index'] = rp_index.clone()
            lin(f'{b}.attn.qkv', 3 * dim, dim)
            lin(f'{b}.attn.proj', dim, dim)
            ln(f'{b}.norm2', dim)
            lin(f'{b}.mlp.fc1', hidden, dim)
            lin(f'{b}.mlp.fc2', dim, hidden)
            _conv(sd, f'layers.{i}.adjust{j}', gc if j < 5 else C, dim, 1, seed)
    ln('norm', C)
    if resi == '1conv':
        _conv(sd, 'conv_after_body', C, C, 3, seed)
    _conv(sd, 'conv_before_upsample.0', 64, C, 3, seed)
    if upscale == 3:
        _conv(sd, 'upsample.0', 9 * 64, 64, 3, seed)
    else:
        for u in range(int(np.log2(upscale))):
            _conv(sd, f'upsample.{2 * u}', 4 * 64, 64, 3, seed)
    _conv(sd, 'conv_last', in_chans, 64, 3, seed)
    return sd


def _plksr_lk(sd, p, pdim, kernel_size, lk_type, seed):
    if lk_type == 'PLK':
        _conv(sd, f'{p}.lk.conv', pdim, pdim, kernel_size, seed)
    elif lk_type == 'RectSparsePLK':
        m, n = kernel_size, kernel_size // 3
        for name, (kh, kw) in (('mn_conv', (m, n)), ('nm_conv', (n, m)), ('nn_conv', (n, n))):
            fan_in = pdim * kh * kw
            sd[f'{p}.lk.{name}.weight'] = synth_tensor(f'{p}.lk.{name}.weight', (pdim, pdim, kh, kw), fan_in, seed)
            sd[f'{p}.lk.{name}.bias'] = synth_tensor(f'{p}.lk.{name}.bias', (pdim,), fan_in, seed)
    elif lk_type == 'SparsePLK':  # the reference loader's fixed sub-kernels: 4 x (5 x 5) at dilations 1..4
        for j in range(4):
            _conv(sd, f'{p}.lk.convs.{j}', pdim, pdim, 5, seed, scale=0.5)
    else:
        raise ValueError(lk_type)


def plksr_state_dict(dim=64, n_blocks=2, upscale=4, ccm_type='DCCM', kernel_size=17, split_ratio=0.25, lk_type='PLK', use_ea=True, seed=0):
    """Keys of PLKSR (archs/plksr/plksr.py:259-318); note the reference's ``channe_mixer`` spelling."""
    sd: OrderedDict = OrderedDict()
    k0, k2 = {'CCM': (3, 1), 'ICCM': (1, 3), 'DCCM': (3, 3)}[ccm_type]
    pdim = int(dim * split_ratio)
    _conv(sd, 'feats.0', dim, 3, 3, seed)
    for b in range(1, n_blocks + 1):
        p = f'feats.{b}'
        _conv(sd, f'{p}.channe_mixer.0', 2 * dim, dim, k0, seed)
        _conv(sd, f'{p}.channe_mixer.2', dim, 2 * dim, k2, seed)
        _plksr_lk(sd, p, pdim, kernel_size, lk_type, seed)
        if use_ea:
            _conv(sd, f'{p}.attn.f.0', dim, dim, 3, seed)
        _conv(sd, f'{p}.refine', dim, dim, 1, seed)
    _conv(sd, f'feats.{n_blocks + 1}', 3 * upscale * upscale, dim, 3, seed)
    return sd


def realplksr_state_dict(dim=64, n_blocks=2, upscale=4, kernel_size=17, split_ratio=0.25, use_ea=True, dysample=False, seed=0):
    """Keys of RealPLKSR (archs/plksr/rplksr.py:108-166): GroupNorm per block, Dropout2d (no keys), PixelShuffle or DySample head."""
    sd: OrderedDict = OrderedDict()
    pdim = int(dim * split_ratio)
    _conv(sd, 'feats.0', dim, 3, 3, seed)
    for b in range(1, n_blocks + 1):
        p = f'feats.{b}'
        _conv(sd, f'{p}.channel_mixer.0', 2 * dim, dim, 3, seed)
        _conv(sd, f'{p}.channel_mixer.2', dim, 2 * dim, 3, seed)
        _conv(sd, f'{p}.lk.conv', pdim, pdim, kernel_size, seed)
        if use_ea:
            _conv(sd, f'{p}.attn.f.0', dim, dim, 3, seed)
        _conv(sd, f'{p}.refine', dim, dim, 1, seed)
        sd[f'{p}.norm.weight'] = 1.0 + synth_tensor(f'{p}.norm.weight', (dim,), 16, seed)
        sd[f'{p}.norm.bias'] = synth_tensor(f'{p}.norm.bias', (dim,), 16, seed)
    cin = 3 * upscale * upscale
    _conv(sd, f'feats.{n_blocks + 2}', cin, dim, 3, seed)
    if dysample:
        groups = 3 if upscale % 2 else 4
        oc = 2 * groups * upscale * upscale
        if upscale != 1:
            _conv(sd, 'to_img.end_conv', 3, cin, 1, seed)
        _conv(sd, 'to_img.offset', oc, cin, 1, seed, scale=0.5)
        _conv(sd, 'to_img.scope', oc, cin, 1, seed, bias=False)
        h = torch.arange((-upscale + 1) / 2, (upscale - 1) / 2 + 1) / upscale
        sd['to_img.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, groups, 1).reshape(1, -1, 1, 1)
    return sd


def cugan_state_dict(variant='2x', pro=False, seed=0):
    """Keys of Real-CUGAN (archs/cugan/arch.py): UpCunet2x / 3x / 4x / 2x_fast ('2x_fast' has no `pro` form).  Transposed convolutions are
    [cin][cout][k][k]; weights are drawn with twice the usual bound so that activations keep their scale through the U-Nets."""
    from ..archs.cugan.arch import param_shapes

    sd: OrderedDict = OrderedDict()
    for name, shape in param_shapes(variant, 3, 3).items():
        if name.endswith('.bias'):
            continue
        layer = name[: -len('.weight')]
        transposed = layer.endswith('_up') or (layer == 'unet1.conv_bottom')
        co, ci = (shape[1], shape[0]) if transposed else (shape[0], shape[1])
        k = shape[2]
        fan_in = ci * k * k // (4 if transposed and k % 2 == 0 else 9 if transposed else 1)
        sd[name] = synth_tensor(name, shape, fan_in, seed, 2.0)
        sd[f'{layer}.bias'] = synth_tensor(f'{layer}.bias', (co,), fan_in, seed, 0.5)
    if pro:
        if variant == '2x_fast':
            raise ValueError('UpCunet2x_fast has no pro form')
        sd['pro'] = torch.zeros(1)
    return sd


def _dwconv(sd, name, c, kh, kw, seed):
    sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (c, 1, kh, kw), kh * kw, seed)
    sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), kh * kw, seed)


def _mosr_trunk(sd, first: int, n_block: int, dim: int, seed) -> None:
    """The three convolutions after the gated blocks (mosr/arch.py:126, mosrv2/arch.py:307-313)."""
    t = first + n_block
    _conv(sd, f'gblocks.{t}', 2 * dim, dim, 3, seed)
    _conv(sd, f'gblocks.{t + 2}', dim, 2 * dim, 3, seed)
    _conv(sd, f'gblocks.{t + 4}', dim, dim, 1, seed)


def mosr_state_dict(in_ch=3, out_ch=3, upscale=4, n_block=24, dim=64, upsampler='ps', kernel_size=7, expansion_ratio=1.5, conv_ratio=1.0, seed=0):
    """Keys of the reference MoSR module (archs/mosr/arch.py:108-156): 'ps', 'dys' or 'gps' head."""
    sd: OrderedDict = OrderedDict()
    if upsampler == 'ps':
        out_ch = in_ch
    hidden = int(expansion_ratio * dim)
    cc = int(conv_ratio * dim)
    _conv(sd, 'gblocks.0', dim, in_ch, 3, seed)
    for i in range(1, n_block + 1):
        b = f'gblocks.{i}'
        sd[f'{b}.norm.weight'] = 1.0 + synth_tensor(f'{b}.norm.weight', (dim,), 16, seed)
        sd[f'{b}.norm.bias'] = synth_tensor(f'{b}.norm.bias', (dim,), 16, seed)
        _conv(sd, f'{b}.fc1', 2 * hidden, dim, 3, seed)
        _dwconv(sd, f'{b}.conv', cc, kernel_size, kernel_size, seed)
        _conv(sd, f'{b}.fc2', dim, hidden, 3, seed)
    _mosr_trunk(sd, 1, n_block, dim, seed)
    _conv(sd, 'shortcut.block.0', dim, in_ch, 3, seed)
    _conv(sd, 'shortcut.block.2', dim, dim, 3, seed)
    _conv(sd, 'shortcut.conv11', dim, in_ch, 1, seed)
    if upsampler == 'ps':
        _conv(sd, 'upsampler.0', out_ch * upscale * upscale, dim, 3, seed)
    elif upsampler == 'dys':
        oc = 8 * upscale * upscale
        _conv(sd, 'upsampler.end_conv', out_ch, dim, 1, seed)
        _conv(sd, 'upsampler.offset', oc, dim, 1, seed, scale=0.5)
        _conv(sd, 'upsampler.scope', oc, dim, 1, seed, bias=False)
        h = torch.arange((-upscale + 1) / 2, (upscale - 1) / 2 + 1) / upscale
        sd['upsampler.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
    elif upsampler == 'gps':
        _conv(sd, 'upsampler.in_to_k', upscale * upscale * out_ch * 8, dim, 3, seed)
    else:
        raise ValueError(f'unknown MoSR upsampler {upsampler!r}')
    return sd


MOSRV2_SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')


def mosrv2_state_dict(in_ch=3, scale=4, n_block=24, dim=64, upsampler='pixelshuffledirect', expansion_ratio=1.5, mid_dim=32, unshuffle_mod=True,
                      rms_norm=False, seed=0):  # fmt: skip
    """Keys of the reference MoSRv2 module (archs/mosrv2/arch.py:281-337), ``to_img.MetaUpsample`` included."""
    sd: OrderedDict = OrderedDict()
    s_int = scale
    if unshuffle_mod and scale < 3:
        u = 4 // scale
        _conv(sd, 'gblocks.1', dim, in_ch * u * u, 3, seed)
        first, s_int = 2, 4
    else:
        _conv(sd, 'gblocks.0', dim, in_ch, 3, seed)
        first = 1
    hidden = int(expansion_ratio * dim)
    gc = int(dim * 0.125)
    for i in range(first, first + n_block):
        b = f'gblocks.{i}'
        if rms_norm:
            sd[f'{b}.norm.scale'] = 1.0 + synth_tensor(f'{b}.norm.scale', (dim, 1, 1), 16, seed)
            sd[f'{b}.norm.offset'] = synth_tensor(f'{b}.norm.offset', (dim, 1, 1), 16, seed)
        else:
            sd[f'{b}.norm.weight'] = 1.0 + synth_tensor(f'{b}.norm.weight', (dim,), 16, seed)
            sd[f'{b}.norm.bias'] = synth_tensor(f'{b}.norm.bias', (dim,), 16, seed)
        _conv(sd, f'{b}.fc1', 2 * hidden, dim, 3, seed)
        _dwconv(sd, f'{b}.conv.dwconv_hw', gc, 3, 3, seed)
        _dwconv(sd, f'{b}.conv.dwconv_w', gc, 1, 11, seed)
        _dwconv(sd, f'{b}.conv.dwconv_h', gc, 11, 1, seed)
        _conv(sd, f'{b}.fc2', dim, hidden, 3, seed)
        sd[f'{b}.gamma'] = 1.0 + synth_tensor(f'{b}.gamma', (1, dim, 1, 1), 16, seed)
    _mosr_trunk(sd, first, n_block, dim, seed)
    up, s = upsampler, s_int
    if s == 1 or up == 'conv':
        _conv(sd, 'to_img.0', in_ch, dim, 3, seed)
    elif up == 'pixelshuffledirect':
        _conv(sd, 'to_img.0', in_ch * s * s, dim, 3, seed)
    elif up == 'pixelshuffle':
        _conv(sd, 'to_img.0', mid_dim, dim, 3, seed)
        i = 2
        for r in [2] * (s.bit_length() - 1) if s & (s - 1) == 0 else [3]:
            _conv(sd, f'to_img.{i}', r * r * mid_dim, mid_dim, 3, seed)
            i += 2
        _conv(sd, f'to_img.{i}', in_ch, mid_dim, 3, seed)
    elif up == 'nearest+conv':
        i = 0
        for _ in range(s.bit_length() - 1 if s & (s - 1) == 0 else 1):
            _conv(sd, f'to_img.{i}', dim, dim, 3, seed)
            i += 3
        _conv(sd, f'to_img.{i}', dim, dim, 3, seed)
        _conv(sd, f'to_img.{i + 2}', in_ch, dim, 3, seed)
    elif up == 'dysample':
        i, dys_dim = 0, dim
        if mid_dim != dim:
            _conv(sd, 'to_img.0', mid_dim, dim, 3, seed)
            i, dys_dim = 2, mid_dim
        oc = 8 * s * s
        _conv(sd, f'to_img.{i}.end_conv', in_ch, dys_dim, 1, seed)
        _conv(sd, f'to_img.{i}.offset', oc, dys_dim, 1, seed, scale=0.5)
        _conv(sd, f'to_img.{i}.scope', oc, dys_dim, 1, seed, bias=False)
        h = torch.arange((-s + 1) / 2, (s - 1) / 2 + 1) / s
        sd[f'to_img.{i}.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
    else:
        raise ValueError(f'unknown MoSRv2 upsampler {up!r}')
    sd['to_img.MetaUpsample'] = torch.tensor([2, MOSRV2_SAMPLE_MODS.index(up), s, dim, in_ch, mid_dim, 4], dtype=torch.uint8)
    return sd


def _uni_upsample(sd, prefix, up, s, dim, out_ch, mid_dim, seed, version):
    """UniUpsample as MoESR registers it (archs/moesr/arch.py:14-88): the MetaUpsample buffer first, DySample on the features themselves."""
    sd[f'{prefix}.MetaUpsample'] = torch.tensor([version, MOSRV2_SAMPLE_MODS.index(up), s, dim, out_ch, mid_dim, 4], dtype=torch.uint8)
    if s == 1 or up == 'conv':
        _conv(sd, f'{prefix}.0', out_ch, dim, 3, seed)
    elif up == 'pixelshuffledirect':
        _conv(sd, f'{prefix}.0', out_ch * s * s, dim, 3, seed)
    elif up == 'pixelshuffle':
        _conv(sd, f'{prefix}.0', mid_dim, dim, 3, seed)
        i = 2
        for r in [2] * (s.bit_length() - 1) if s & (s - 1) == 0 else [3]:
            _conv(sd, f'{prefix}.{i}', r * r * mid_dim, mid_dim, 3, seed)
            i += 2
        _conv(sd, f'{prefix}.{i}', out_ch, mid_dim, 3, seed)
    elif up == 'nearest+conv':
        i = 0
        for _ in range(s.bit_length() - 1 if s & (s - 1) == 0 else 1):
            _conv(sd, f'{prefix}.{i}', dim, dim, 3, seed)
            i += 3
        _conv(sd, f'{prefix}.{i}', dim, dim, 3, seed)
        _conv(sd, f'{prefix}.{i + 2}', out_ch, dim, 3, seed)
    elif up == 'dysample':
        oc = 8 * s * s
        h = torch.arange((-s + 1) / 2, (s - 1) / 2 + 1) / s  # (DySample's own buffer: before its sub-modules)
        sd[f'{prefix}.0.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
        _conv(sd, f'{prefix}.0.end_conv', out_ch, dim, 1, seed)
        _conv(sd, f'{prefix}.0.offset', oc, dim, 1, seed, scale=0.5)
        _conv(sd, f'{prefix}.0.scope', oc, dim, 1, seed, bias=False)
    else:
        raise ValueError(f'unknown UniUpsample mode {up!r}')


def moesr_state_dict(in_ch=3, out_ch=3, scale=4, dim=64, n_blocks=9, n_block=4, expansion_factor=8 / 3, expansion_msg=1.5,
                     upsampler='pixelshuffledirect', upsample_dim=64, seed=0):  # fmt: skip
    """Keys of the reference MoESR module (archs/moesr/arch.py:190-227) in its registration order: a block's ``gamma`` (its own parameter)
    before its sub-modules, ``upscale.MetaUpsample`` before the head's layers.  ``gamma`` is 1 + uniform(+-0.25), so the scale is exercised;
    the two convolutions of an MSG are drawn at half the default bound, which keeps the default depth (63 blocks) of order 1."""
    sd: OrderedDict = OrderedDict()
    if upsampler == 'conv':
        scale = 1
    gc = int(dim * 0.125)

    def block(b, hidden):
        sd[f'{b}.gamma'] = 1.0 + synth_tensor(f'{b}.gamma', (1, dim, 1, 1), 16, seed)
        sd[f'{b}.norm.weight'] = 1.0 + synth_tensor(f'{b}.norm.weight', (dim,), 16, seed)
        sd[f'{b}.norm.bias'] = synth_tensor(f'{b}.norm.bias', (dim,), 16, seed)
        _conv(sd, f'{b}.fc1', 2 * hidden, dim, 3, seed)
        _dwconv(sd, f'{b}.conv.dwconv_hw', gc, 3, 3, seed)
        _dwconv(sd, f'{b}.conv.dwconv_w', gc, 1, 11, seed)
        _dwconv(sd, f'{b}.conv.dwconv_h', gc, 11, 1, seed)
        _conv(sd, f'{b}.fc2', dim, hidden, 3, seed)

    _conv(sd, 'in_to_dim', dim, in_ch, 3, seed)
    for g in range(n_blocks):
        for j in range(n_block):
            block(f'blocks.{g}.blocks.{j}', int(expansion_factor * dim))
        m = f'blocks.{g}.msg'
        _conv(sd, f'{m}.down.0', dim // 4, dim, 3, seed, scale=0.5)
        for j in range(3):
            block(f'{m}.gated.{j}', int(expansion_msg * dim))
        _conv(sd, f'{m}.up.0', 4 * dim, dim, 3, seed, scale=0.5)
    _uni_upsample(sd, 'upscale', upsampler, scale, dim, out_ch, upsample_dim, seed, version=1)
    return sd


def rgt_state_dict(in_chans=3, embed_dim=48, split_size=(2, 4), depth=(2,), num_heads=(4,), mlp_ratio=2.0, qkv_bias=True, upscale=2, resi='1conv',
                   c_ratio=0.5, img_size=64, seed=0):  # fmt: skip
    """Keys (parameters AND buffers) of the reference RGT module (archs/rgt/arch.py:630-838).

    Every term is made visible: the HAI ``gamma`` is of order 0.1-1 (not the 1e-4 init), LayerNorm affines and the position-bias MLPs are
    non-trivial, and ``reduction1`` is about 1/16 per tap so that t repeats of it neither vanish nor blow up.
    """
    sd: OrderedDict = OrderedDict()
    C = embed_dim
    hidden = int(C * mlp_ratio)
    cr = int(C * c_ratio)
    split_size = list(split_size)
    shift_size = [split_size[0] // 2, split_size[1] // 2]

    def lin(name, cout, cin, bias=True):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (cout, cin), cin, seed)
        if bias:
            sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (cout,), cin, seed)

    def ln(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), 16, seed)

    def dw(name, c, k=3, scale=1.0):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (c, 1, k, k), k * k, seed, scale)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), k * k, seed, scale)

    def window_branch(name, idx, heads):
        hs, ws = dat_geometry(split_size, idx)
        bh, bw = torch.arange(1 - hs, hs), torch.arange(1 - ws, ws)
        sd[f'{name}.rpe_biases'] = torch.stack(torch.meshgrid([bh, bw], indexing='ij')).flatten(1).transpose(0, 1).contiguous().float()
        coords = torch.stack(torch.meshgrid([torch.arange(hs), torch.arange(ws)], indexing='ij')).flatten(1)
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += hs - 1
        rel[:, :, 1] += ws - 1
        rel[:, :, 0] *= 2 * ws - 1
        sd[f'{name}.relative_position_index'] = rel.sum(-1)
        pos_dim = ((C // 2) // 4) // 4  # WindowAttention(dim // 2) -> DynamicPosBias(dim // 4) -> pos_dim = dim // 4 (arch.py:103, 164)
        lin(f'{name}.pos.pos_proj', pos_dim, 2)
        for k, cout in (('pos1', pos_dim), ('pos2', pos_dim), ('pos3', heads)):
            sd[f'{name}.pos.{k}.0.weight'] = 1.0 + synth_tensor(f'{name}.pos.{k}.0.weight', (pos_dim,), 16, seed)
            sd[f'{name}.pos.{k}.0.bias'] = synth_tensor(f'{name}.pos.{k}.0.bias', (pos_dim,), 16, seed)
            lin(f'{name}.pos.{k}.2', cout, pos_dim)

    _conv(sd, 'conv_first', C, in_chans, 3, seed)
    ln('before_RG.1', C)
    for i, d in enumerate(depth):
        heads = num_heads[i]
        for j in range(d):
            b = f'layers.{i}.blocks.{j}'
            ln(f'{b}.norm1', C)
            if j % 2 == 0:  # L_SA
                lin(f'{b}.attn.qkv', 3 * C, C, qkv_bias)
                lin(f'{b}.attn.proj', C, C)
                for idx in (0, 1):
                    window_branch(f'{b}.attn.attns.{idx}', idx, heads // 2)
                if dat_shifted(i, j):
                    m0, m1 = dat_shift_masks(img_size, img_size, split_size, shift_size)
                    sd[f'{b}.attn.attn_mask_0'] = m0
                    sd[f'{b}.attn.attn_mask_1'] = m1
                dw(f'{b}.attn.get_v', C)
            else:  # RG_SA
                sd[f'{b}.attn.reduction1.weight'] = (1.0 + 8.0 * synth_tensor(f'{b}.attn.reduction1.weight', (C, 1, 4, 4), 16, seed)) / 16.0
                sd[f'{b}.attn.reduction1.bias'] = synth_tensor(f'{b}.attn.reduction1.bias', (C,), 16, seed, 0.5)
                dw(f'{b}.attn.dwconv', C)
                _conv(sd, f'{b}.attn.conv', cr, C, 1, seed)
                ln(f'{b}.attn.norm_act.0', cr)
                lin(f'{b}.attn.q', cr, C, qkv_bias)
                lin(f'{b}.attn.k', cr, cr, qkv_bias)
                lin(f'{b}.attn.v', C, cr, qkv_bias)
                dw(f'{b}.attn.cpe', C)
                lin(f'{b}.attn.proj', C, C)
            lin(f'{b}.mlp.fc1', hidden, C)
            ln(f'{b}.mlp.sg.norm', hidden // 2)
            dw(f'{b}.mlp.sg.conv', hidden // 2)
            lin(f'{b}.mlp.fc2', C, hidden // 2)
            ln(f'{b}.norm2', C)
            sd[f'{b}.gamma'] = 0.55 + synth_tensor(f'{b}.gamma', (C,), 1, seed, 0.45)
        _resi_conv(sd, f'layers.{i}.conv', C, resi, seed)
    ln('norm', C)
    _resi_conv(sd, 'conv_after_body', C, resi, seed)
    _conv(sd, 'conv_before_upsample.0', 64, C, 3, seed)
    if upscale == 3:
        _conv(sd, 'upsample.0', 9 * 64, 64, 3, seed)
    else:
        for u in range({1: 0, 2: 1, 4: 2, 8: 3}[upscale]):
            _conv(sd, f'upsample.{2 * u}', 4 * 64, 64, 3, seed)
    _conv(sd, 'conv_last', in_chans, 64, 3, seed)
    return sd


FDAT_SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')


def fdat_state_dict(num_in_ch=3, num_out_ch=3, scale=4, embed_dim=48, num_groups=1, depth_per_group=1, num_heads=4, window_size=4,
                    ffn_expansion_ratio=2.0, aim_reduction_ratio=8, mid_dim=32, upsampler_type='transpose+conv', unshuffle_mod=False, seed=0):  # fmt: skip
    """Keys of the reference FDAT module (archs/fdat/arch.py:632-735), ``upsampler.MetaUpsample`` included (LDA's ``base_offset`` is not
    persistent).  The window bias, the channel-attention temperature, the AIM gates and the LDA offsets are of visible size; the LDA offset
    convolution is scaled so that tanh(o) * 11 spans a few pixels without saturating."""
    sd: OrderedDict = OrderedDict()
    C = embed_dim
    hidden = int(C * ffn_expansion_ratio)
    red = C // aim_reduction_ratio
    s = scale
    if unshuffle_mod and scale < 3:
        u = 4 // scale
        _conv(sd, 'conv_first.1', C, num_in_ch * u * u, 3, seed)
        s = 4
    else:
        _conv(sd, 'conv_first', C, num_in_ch, 3, seed)

    def t(name, shape, fan_in, scale_=1.0):
        sd[name] = synth_tensor(name, shape, fan_in, seed, scale_)

    for g in range(num_groups):
        for j in range(2 * depth_per_group):
            b = f'groups.{g}.blocks.{j}'
            for nrm in ('n1', 'n2'):
                sd[f'{b}.{nrm}.weight'] = 1.0 + synth_tensor(f'{b}.{nrm}.weight', (C,), 16, seed)
                t(f'{b}.{nrm}.bias', (C,), 16)
            if j % 2 == 0:
                t(f'{b}.attn.bias', (num_heads, window_size**2, window_size**2), 4)
            else:
                sd[f'{b}.attn.temp'] = 1.0 + synth_tensor(f'{b}.attn.temp', (num_heads, 1, 1), 4, seed)
            t(f'{b}.attn.qkv.weight', (3 * C, C), C)
            t(f'{b}.attn.proj.weight', (C, C), C)
            t(f'{b}.attn.proj.bias', (C,), C)
            t(f'{b}.conv.0.weight', (C, 1, 3, 3), 9)
            t(f'{b}.inter.sg.0.weight', (1, C, 1, 1), C)
            t(f'{b}.inter.cg.1.weight', (red, C, 1, 1), C, 2.0)
            t(f'{b}.inter.cg.3.weight', (C, red, 1, 1), red, 2.0)
            t(f'{b}.ffn.fc1.weight', (hidden, C), C)
            t(f'{b}.ffn.fc2.weight', (C, hidden), hidden)
            t(f'{b}.ffn.smix.weight', (hidden, 1, 3, 3), 9)
        t(f'groups.{g}.conv.weight', (C, C, 3, 3), 9 * C)
    t('conv_after.weight', (C, C, 3, 3), 9 * C)
    up, out, mid = upsampler_type, num_out_ch, mid_dim
    sd['upsampler.MetaUpsample'] = torch.tensor([3, FDAT_SAMPLE_MODS.index(up), s, C, out, mid, 4], dtype=torch.uint8)
    pow2 = s & (s - 1) == 0
    if s == 1 or up == 'conv':
        _conv(sd, 'upsampler.0', out, C, 3, seed)
    elif up == 'pixelshuffledirect':
        _conv(sd, 'upsampler.0', out * s * s, C, 3, seed)
    elif up == 'pixelshuffle':
        _conv(sd, 'upsampler.0', mid, C, 3, seed)
        i = 2
        for r in [2] * (s.bit_length() - 1) if pow2 else [3]:
            _conv(sd, f'upsampler.{i}', r * r * mid, mid, 3, seed)
            i += 2
        _conv(sd, f'upsampler.{i}', out, mid, 3, seed)
    elif up == 'nearest+conv':
        i = 0
        for _ in range(s.bit_length() - 1 if pow2 else 1):
            _conv(sd, f'upsampler.{i}', C, C, 3, seed)
            i += 3
        _conv(sd, f'upsampler.{i}', C, C, 3, seed)
        _conv(sd, f'upsampler.{i + 2}', out, C, 3, seed)
    elif up == 'dysample':
        i, dys_dim = 0, C
        if mid != C:
            _conv(sd, 'upsampler.0', mid, C, 3, seed)
            i, dys_dim = 2, mid
        oc = 8 * s * s
        _conv(sd, f'upsampler.{i}.end_conv', out, dys_dim, 1, seed)
        _conv(sd, f'upsampler.{i}.offset', oc, dys_dim, 1, seed, scale=0.5)
        _conv(sd, f'upsampler.{i}.scope', oc, dys_dim, 1, seed, bias=False)
        h = torch.arange((-s + 1) / 2, (s - 1) / 2 + 1) / s
        sd[f'upsampler.{i}.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
    elif up == 'transpose+conv':
        def deconv(name, cin, cout, k):
            t(f'{name}.weight', (cin, cout, k, k), cin * k * k // 4)
            t(f'{name}.bias', (cout,), cin)

        if s == 2:
            deconv('upsampler.0', C, out, 4)
        elif s == 3:
            deconv('upsampler.0', C, out, 3)
        else:
            deconv('upsampler.0', C, C, 4)
            deconv('upsampler.2', C, out, 4)
        _conv(sd, f'upsampler.{1 if s < 4 else 3}', out, out, 3, seed)
    elif up == 'lda':
        i = 0
        if mid != C:
            _conv(sd, 'upsampler.0', mid, C, 3, seed)
            i = 2
        u = f'upsampler.{i}'
        hid, gc = mid // 4, mid // 8
        t(f'{u}.relative_position_bias_table', (1, 1, 1, 9, hid), 4, 0.5)
        t(f'{u}.proj_q.weight', (hid, mid, 1, 1), mid, 2.0)
        t(f'{u}.proj_k.weight', (hid, mid, 1, 1), mid, 2.0)
        t(f'{u}.conv_offset.0.weight', (gc, 1, 3, 3), 9)
        sd[f'{u}.conv_offset.1.weight'] = 1.0 + synth_tensor(f'{u}.conv_offset.1.weight', (gc,), 16, seed)
        t(f'{u}.conv_offset.1.bias', (gc,), 16)
        _conv(sd, f'{u}.conv_offset.3', 18, gc, 3, seed, scale=0.3)
        sd[f'{u}.layer_norm.weight'] = 1.0 + synth_tensor(f'{u}.layer_norm.weight', (mid,), 16, seed)
        t(f'{u}.layer_norm.bias', (mid,), 16)
        _conv(sd, f'upsampler.{i + 1}', out, mid, 3, seed)
    elif up == 'pa_up':
        i, cin = 0, C
        for _ in range(s.bit_length() - 1 if pow2 else 1):
            _conv(sd, f'upsampler.{i + 1}', mid, cin, 3, seed)
            _conv(sd, f'upsampler.{i + 2}.conv.0', mid, mid, 1, seed)
            _conv(sd, f'upsampler.{i + 4}', mid, mid, 3, seed)
            i, cin = i + 6, mid
        _conv(sd, f'upsampler.{i}', out, mid, 3, seed)
    else:
        raise ValueError(f'unknown FDAT upsampler {up!r}')
    return sd


def omnisr_state_dict(num_in_ch=3, num_feat=64, res_num=1, block_num=1, pe=True, window_size=8, up_scale=4, bias=True, seed=0):
    """Keys of the reference OmniSR module (archs/omni/arch.py:907-974).  LayerNorm weights sit around 1, the channel-attention temperatures
    around 1 and the relative-position bias tables are of visible size."""
    from ..archs.omnisr.arch import omnisr_param_shapes

    sd: OrderedDict = OrderedDict()
    shapes = omnisr_param_shapes(num_in_ch, num_in_ch, num_feat, res_num, block_num, window_size, pe, up_scale, bias)
    for name, shape in shapes.items():
        if name.endswith('norm.weight'):
            sd[name] = 1.0 + synth_tensor(name, shape, 16, seed)
        elif name.endswith('norm.bias'):
            sd[name] = synth_tensor(name, shape, 16, seed)
        elif name.endswith('temperature'):
            sd[name] = 1.0 + synth_tensor(name, shape, 1, seed, 0.5)
        elif name.endswith('rel_pos_bias.weight'):
            sd[name] = synth_tensor(name, shape, 1, seed)
        elif name.endswith('.weight'):
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            sd[name] = synth_tensor(name, shape, fan_in, seed)
        else:  # a bias: the fan-in of its weight
            w = shapes[name[: -len('bias')] + 'weight']
            sd[name] = synth_tensor(name, shape, int(np.prod(w[1:])), seed)
    return sd


def atd_state_dict(in_chans=3, embed_dim=48, depths=(2, 2), num_heads=(4, 4), window_size=8, num_tokens=64, reducted_dim=8, convffn_kernel_size=5,
                   mlp_ratio=2.0, qkv_bias=True, patch_norm=True, upscale=2, upsampler='pixelshuffledirect', resi_connection='1conv', norm=True,
                   seed=0):  # fmt: skip
    """Keys of the reference ATD module (archs/atd/arch.py:829-1010).  The dictionary, wq and wk are of visible size, so the similarity maps
    are far from uniform (cosine logits span about +-(1 + ln m / 2)); LayerNorm / InstanceNorm weights sit around 1; outputs stay of order 1."""
    from ..archs.atd.arch import atd_param_shapes

    sd: OrderedDict = OrderedDict()
    shapes, buffers = atd_param_shapes(in_chans, embed_dim, list(depths), list(num_heads), window_size, num_tokens, reducted_dim, convffn_kernel_size,
                                       mlp_ratio, qkv_bias, patch_norm, upscale, upsampler, resi_connection, norm)  # fmt: skip
    for name, value in buffers.items():
        sd[name] = value.clone()
    for name, shape in shapes.items():
        leaf = name.rsplit('.', 1)[-1]
        if leaf == 'td':
            sd[name] = synth_tensor(name, shape, 1, seed)
        elif leaf == 'sigma':
            sd[name] = synth_tensor(name, shape, 1, seed)
        elif name.endswith('attn_atd.scale'):
            sd[name] = 0.5 + synth_tensor(name, shape, 1, seed, 0.7)  # some entries leave [0, 1]: the clamp is exercised
        elif leaf == 'logit_scale':
            sd[name] = float(np.log(10.0)) + synth_tensor(name, shape, 1, seed, 0.5)
        elif leaf == 'relative_position_bias_table':
            sd[name] = synth_tensor(name, shape, 1, seed)
        elif '.norm' in name and leaf == 'weight' or name in ('norm.weight', 'patch_embed.norm.weight'):
            sd[name] = 1.0 + synth_tensor(name, shape, 16, seed)
        elif '.norm' in name and leaf == 'bias' or name in ('norm.bias', 'patch_embed.norm.bias'):
            sd[name] = synth_tensor(name, shape, 16, seed)
        elif '.wq.' in name or '.wk.' in name:
            sd[name] = synth_tensor(name, shape, int(np.prod(shapes[name[: -len(leaf)] + 'weight'][1:])), seed, 2.0)
        elif leaf == 'weight':
            sd[name] = synth_tensor(name, shape, int(np.prod(shape[1:])) if len(shape) > 1 else 1, seed)
        else:  # a bias: the fan-in of its weight
            sd[name] = synth_tensor(name, shape, int(np.prod(shapes[name[: -len('bias')] + 'weight'][1:])), seed)
    return sd


def rcan_state_dict(scale=4, n_resgroups=2, n_resblocks=2, n_feats=64, n_colors=3, reduction=16, norm=True, unshuffle_mod=False, kernel_size=3, seed=0):
    """Keys of RCAN (archs/rcan/arch.py:236-332) in the module's registration order: sub_mean / add_mean (with ``norm``), head, the residual
    groups of RCABs (two convolutions and the channel attention's conv_du pair), each group's and the body's closing convolution, the
    Upsampler stack and the last convolution.  The mean shifts are full 3x3 matrices near the DIV2K ones (an identity plus a perturbation), so
    that nothing downstream can get away with assuming a diagonal.  The module's MeanShift is nn.Conv2d(3, 3, 1) whatever ``n_colors`` is
    (:48), so ``norm`` needs three channels -- in the reference too, whose forward fails on anything else."""
    sd: OrderedDict = OrderedDict()
    if norm and n_colors != 3:
        raise ValueError('rcan_state_dict: norm=True needs n_colors == 3 (the mean shifts are 3 -> 3 convolutions)')
    if norm:
        eye = torch.eye(n_colors).view(n_colors, n_colors, 1, 1)
        mean = 255.0 * torch.tensor((0.4488, 0.4371, 0.4040, 0.43)[:n_colors])
        for name, sign in (('sub_mean', -1.0), ('add_mean', 1.0)):
            sd[f'{name}.weight'] = eye + 0.1 * synth_tensor(f'{name}.weight', (n_colors, n_colors, 1, 1), n_colors, seed)
            sd[f'{name}.bias'] = sign * mean + synth_tensor(f'{name}.bias', (n_colors,), 1, seed)
    down = 4 // scale if (unshuffle_mod and scale <= 2) else 1
    _conv(sd, 'head.1' if down > 1 else 'head.0', n_feats, n_colors * down * down, kernel_size, seed)
    for g in range(n_resgroups):
        for b in range(n_resblocks):
            p = f'body.{g}.body.{b}.body'
            _conv(sd, f'{p}.0', n_feats, n_feats, kernel_size, seed)
            _conv(sd, f'{p}.2', n_feats, n_feats, kernel_size, seed)
            _conv(sd, f'{p}.3.conv_du.0', n_feats // reduction, n_feats, 1, seed)
            _conv(sd, f'{p}.3.conv_du.2', n_feats, n_feats // reduction, 1, seed)
        _conv(sd, f'body.{g}.body.{n_resblocks}', n_feats, n_feats, kernel_size, seed)
    _conv(sd, f'body.{n_resgroups}', n_feats, n_feats, kernel_size, seed)
    net_scale = 4 if down > 1 else scale
    if net_scale == 3:
        _conv(sd, 'tail.0.0', 9 * n_feats, n_feats, 3, seed)
    else:
        for i in range(int(np.log2(net_scale))):
            _conv(sd, f'tail.0.{2 * i}', 4 * n_feats, n_feats, 3, seed)
    _conv(sd, 'tail.1', n_colors, n_feats, kernel_size, seed)
    return sd


def gater_state_dict(dim=48, in_ch=3, num_blocks=(3, 6, 6, 10, 6, 6, 3), latent_att=False, seed=0):
    """Keys of GateR (archs/gater/arch.py:162-200) in the module's registration order.  Matrices and filters are uniform with variance
    1 / fan_in (roughly unit gain through a block), norm weights lie in 0.5..1.5, biases in +-0.09.  The latent attention's ``scale`` and
    ``focusing_factor`` are drawn PER CHANNEL (+-0.87 and 2..4): the module's own initialisation leaves them constant, which would hide a
    per-channel indexing error.  The last convolution is scaled by 0.1 so that the output stays near the image range."""
    sd: OrderedDict = OrderedDict()
    g = float(np.sqrt(3.0))  # uniform(-g / sqrt(fan_in), ..): variance 1 / fan_in

    def lin(name, co, ci):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci), ci, seed, g)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (co,), 1, seed, 0.05 * g)

    def conv(name, co, ci, k, groups=1, gain=1.0):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci // groups, k, k), (ci // groups) * k * k, seed, g * gain)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (co,), 1, seed, 0.05 * g * gain)

    def blocks(prefix, width, n, att=False):
        hidden = int((1.5 if att else 8 / 3) * width)
        for i in range(n):
            b = f'{prefix}.gated.{i}'
            sd[f'{b}.norm.weight'] = 1.0 + synth_tensor(f'{b}.norm.weight', (width,), 1, seed, 0.5)
            lin(f'{b}.fc1', 2 * hidden, width)
            if att:
                sd[f'{b}.conv.focusing_factor'] = 3.0 + synth_tensor(f'{b}.conv.focusing_factor', (width,), 1, seed, 1.0)
                sd[f'{b}.conv.scale'] = synth_tensor(f'{b}.conv.scale', (width,), 1, seed, 0.5 * g)
                lin(f'{b}.conv.q', width, width)
                lin(f'{b}.conv.kv', 2 * width, width)
                lin(f'{b}.conv.proj', width, width)
                conv(f'{b}.conv.dwc', width // 8, width // 8, 5, groups=width // 8)
            else:
                conv(f'{b}.conv.conv', width, width, 7, groups=width)
            lin(f'{b}.fc2', width, hidden)

    nb = tuple(num_blocks)
    conv('in_to_dim', dim, in_ch, 3)
    blocks('enc0', dim, nb[0])
    conv('enc1.0.body.0', dim // 2, dim, 3)
    blocks('enc1.1', 2 * dim, nb[1])
    conv('enc2.0.body.0', dim, 2 * dim, 3)
    blocks('enc2.1', 4 * dim, nb[2])
    conv('latent.0.body.0', 2 * dim, 4 * dim, 3)
    blocks('latent.1', 8 * dim, nb[3], latent_att)
    conv('latent.2.body.0', 16 * dim, 8 * dim, 3)
    conv('dec0.0', 4 * dim, 8 * dim, 1)
    blocks('dec0.1', 4 * dim, nb[4])
    conv('dec0.2.body.0', 8 * dim, 4 * dim, 3)
    conv('dec1.0', 2 * dim, 4 * dim, 1)
    blocks('dec1.1', 2 * dim, nb[5])
    conv('dec1.2.body.0', 4 * dim, 2 * dim, 3)
    blocks('dec2.0', 2 * dim, nb[6])
    conv('dim_to_ch.0', dim, 2 * dim, 3)
    conv('dim_to_ch.1', in_ch, dim, 3, gain=0.1)
    return sd


def eimn_state_dict(embed_dims=64, scale=2, depths=1, hidden=None, mlp_ratios=2.66, num_stages=2, seed=0):
    """Keys of EIMN (archs/eimn/arch.py:174-241) in the module's registration order: head, tail, then per stage its blocks and its LayerNorm.
    ``hidden`` defaults to the reference's ``int(embed_dims * mlp_ratios)``.  Matrices and filters are uniform with variance 1 / fan_in, every
    bias is non-zero (+-0.09).  BatchNorm: weights in 0.5..1.5, running variances in 0.5..1.5, running means about +-0.3,
    ``num_batches_tracked`` 100.  The layer scales lie in 0.1..0.6 -- the module initialises them to 1e-2, which would hide the blocks
    behind the residual -- and the norm weights in 0.5..1.5."""
    sd: OrderedDict = OrderedDict()
    dim = embed_dims
    hidden = int(dim * mlp_ratios) if hidden is None else hidden
    rc = int(dim * 0.25)
    c1, c3 = int(3 / 8 * dim), int(4 / 8 * dim)
    g = float(np.sqrt(3.0))  # uniform(-g / sqrt(fan_in), ..): variance 1 / fan_in

    def conv(name, co, ci, k, groups=1):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci // groups, k, k), (ci // groups) * k * k, seed, g)
        b = synth_tensor(f'{name}.bias', (co,), 1, seed, 0.08 * g)
        sd[f'{name}.bias'] = b + 0.01 * torch.where(b >= 0, 1.0, -1.0)  # never zero

    def affine(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 1, seed, 0.5)
        b = synth_tensor(f'{name}.bias', (c,), 1, seed, 0.08 * g)
        sd[f'{name}.bias'] = b + 0.01 * torch.where(b >= 0, 1.0, -1.0)

    def bn(name):
        affine(name, dim)
        sd[f'{name}.running_mean'] = synth_tensor(f'{name}.running_mean', (dim,), 1, seed, 0.3)
        sd[f'{name}.running_var'] = 1.0 + synth_tensor(f'{name}.running_var', (dim,), 1, seed, 0.5)
        sd[f'{name}.num_batches_tracked'] = torch.tensor(100, dtype=torch.long)

    conv('head.0', dim, 3, 3)
    conv('tail.0', 3 * scale * scale, dim, 3)
    for i in range(1, num_stages + 1):
        for j in range(depths):
            p = f'block{i}.{j}'
            for k in (1, 2):
                sd[f'{p}.layer_scale_{k}'] = 0.35 + synth_tensor(f'{p}.layer_scale_{k}', (dim,), 1, seed, 0.25)
            bn(f'{p}.norm1')
            conv(f'{p}.attn.region', dim, dim, 5, groups=dim)
            conv(f'{p}.attn.spatial_1', c1, c1, 5, groups=c1)
            conv(f'{p}.attn.spatial_2', c3, c3, 7, groups=c3)
            conv(f'{p}.attn.fusion', dim, dim, 1)
            conv(f'{p}.attn.proj_value.0', dim, dim, 1)
            conv(f'{p}.attn.proj_query.0', dim, dim, 1)
            conv(f'{p}.attn.out', dim, dim, 1)
            bn(f'{p}.norm2')
            conv(f'{p}.mlp.linear_in', 2 * hidden, dim, 1)
            conv(f'{p}.mlp.SAL', 2 * hidden, 2 * hidden, 3, groups=2 * hidden)
            conv(f'{p}.mlp.linear_out', dim, hidden, 1)
            q = f'{p}.mlp.DFFM'
            affine(f'{q}.norm', dim)
            conv(f'{q}.global_reduce', rc, dim, 1)
            conv(f'{q}.local_reduce', rc, dim, 1)
            conv(f'{q}.channel_expand', dim, rc, 1)
            conv(f'{q}.spatial_expand', 1, 2 * rc, 1)
        affine(f'norm{i}', dim)
    return sd


RHA_SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')


def rha_state_dict(dim=64, scale=4, in_ch=3, out_ch=3, mid_dim=32, down_list=(8, 4), expansion_ratio=1.5, group_blocks=4, res_blocks=6,
                   upsample='pixelshuffledirect', window_size=8, seed=0):  # fmt: skip
    """Keys of RHA (archs/rha/arch.py:483-565, without ``unshuffle_mod``) in the module's registration order, buffers included: every group's
    ``down_sample``, ``to_img.MetaUpsample`` and the ``conv5x5_reparam`` pair of every OmniShift (which the reference overwrites from the
    training parameters when it enters eval mode: the stored pair is drawn independently here, so that reading it shows).  Matrices and
    filters are uniform with variance 1 / fan_in (fc2: a quarter of that), every bias is non-zero (+-0.09), norm weights lie in 0.5..1.5.
    The attention's ``scale`` is drawn PER CHANNEL in +-1 (softplus 0.31..1.31), ``positional_encoding`` in +-0.5 and the OmniShift
    ``alpha``s in 0.75..1.25: the module initialises them to constants, which would hide a per-channel or per-token indexing error."""
    sd: OrderedDict = OrderedDict()
    g = float(np.sqrt(3.0))  # uniform(-g / sqrt(fan_in), ..): variance 1 / fan_in
    hidden = int(expansion_ratio * dim)
    c2 = dim // 2
    n_tok = window_size * window_size

    def bias(name, co, gain=1.0):
        b = synth_tensor(name, (co,), 1, seed, 0.08 * g * gain)
        return b + 0.01 * gain * torch.where(b >= 0, 1.0, -1.0)  # never zero

    def conv(name, co, ci, k, groups=1, gain=1.0, with_bias=True):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci // groups, k, k), (ci // groups) * k * k, seed, g * gain)
        if with_bias:
            sd[f'{name}.bias'] = bias(f'{name}.bias', co, gain)

    def lin(name, co, ci):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci), ci, seed, g)
        sd[f'{name}.bias'] = bias(f'{name}.bias', co)

    def omnishift(name, c):
        for k in (1, 2, 3, 4):
            sd[f'{name}.alpha{k}'] = 1.0 + synth_tensor(f'{name}.alpha{k}', (1, c, 1, 1), 1, seed, 0.25)
        for sub, ks in (('conv1x1', 1), ('conv3x3', 3), ('conv5x5', 5), ('conv5x5_reparam', 5)):
            conv(f'{name}.{sub}', c, c, ks, groups=c, gain=0.5)

    conv('to_feat', dim, in_ch, 3)
    for gi in range(group_blocks):
        grp = f'body.{gi}'
        sd[f'{grp}.down_sample'] = torch.tensor(down_list[gi % len(down_list)], dtype=torch.uint8)
        for bi in range(res_blocks):
            b = f'{grp}.body.{bi}'
            sd[f'{b}.norm.weight'] = 1.0 + synth_tensor(f'{b}.norm.weight', (dim,), 1, seed, 0.5)
            sd[f'{b}.norm.bias'] = bias(f'{b}.norm.bias', dim)
            conv(f'{b}.fc1', 2 * hidden, dim, 3)
            a = f'{b}.conv.att.2'
            sd[f'{a}.scale'] = synth_tensor(f'{a}.scale', (1, 1, c2), 1, seed, 1.0)
            sd[f'{a}.positional_encoding'] = synth_tensor(f'{a}.positional_encoding', (1, n_tok, c2), 1, seed, 0.5)
            lin(f'{a}.qkv', 3 * c2, c2)
            lin(f'{a}.proj', c2, c2)
            conv(f'{a}.dwc', c2 // 8, c2 // 8, 5, groups=c2 // 8)
            omnishift(f'{b}.conv.conv', c2)
            conv(f'{b}.conv.aggr.0', dim, dim, 1)
            conv(f'{b}.fc2', dim, hidden, 3, gain=0.5)
        omnishift(f'{grp}.body.{res_blocks}', dim)
        conv(f'{grp}.body.{res_blocks + 1}', dim, dim, 1, gain=0.5)
    up, s = upsample, scale
    if up not in RHA_SAMPLE_MODS:
        raise ValueError(f'unknown RHA upsampler {up!r}')
    sd['to_img.MetaUpsample'] = torch.tensor([2, RHA_SAMPLE_MODS.index(up), s, dim, out_ch, mid_dim, 4], dtype=torch.uint8)
    pow2 = s & (s - 1) == 0
    if s == 1 or up == 'conv':
        conv('to_img.0', out_ch, dim, 3, gain=0.2)
    elif up == 'pixelshuffledirect':
        conv('to_img.0', out_ch * s * s, dim, 3, gain=0.2)
    elif up == 'pixelshuffle':
        conv('to_img.0', mid_dim, dim, 3)
        i = 2
        for r in [2] * (s.bit_length() - 1) if pow2 else [3]:
            conv(f'to_img.{i}', r * r * mid_dim, mid_dim, 3)
            i += 2
        conv(f'to_img.{i}', out_ch, mid_dim, 3, gain=0.2)
    elif up == 'nearest+conv':
        i = 0
        for _ in range(s.bit_length() - 1 if pow2 else 1):
            conv(f'to_img.{i}', dim, dim, 3)
            i += 3
        conv(f'to_img.{i}', dim, dim, 3)
        conv(f'to_img.{i + 2}', out_ch, dim, 3, gain=0.2)
    else:
        i, dys_dim = 0, dim
        if mid_dim != dim:
            conv('to_img.0', mid_dim, dim, 3)
            i, dys_dim = 2, mid_dim
        oc = 8 * s * s
        h = torch.arange((-s + 1) / 2, (s - 1) / 2 + 1) / s
        sd[f'to_img.{i}.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
        conv(f'to_img.{i}.end_conv', out_ch, dys_dim, 1, gain=0.2)
        conv(f'to_img.{i}.offset', oc, dys_dim, 1, gain=0.5)
        conv(f'to_img.{i}.scope', oc, dys_dim, 1, with_bias=False)
    return sd


FLEXNET_UPSAMPLERS = ('ps', 'dys', 'n+c')


def flexnet_state_dict(seed=0, dim=64, num_blocks=(6, 6, 6, 6, 6, 6), scale=4, inp_channels=3, out_channels=3, hidden_rate=4, channel_norm=False,
                       upsampler='ps'):  # fmt: skip
    """Keys of FlexNet's linear pipeline (archs/flexnet/arch.py:437-489) in the module's registration order, buffers included: ``window_size``
    (always 8: the only size the reference runs), ``scale_factor`` for ``n+c``, DySample's ``init_pos``, and the ``conv5x5_reparam`` weight of
    every OmniShift, which the reference overwrites from the training parameters on its first forward: the stored one is drawn independently
    here, so that reading it shows.  Matrices and filters are uniform with variance 1 / fan_in, every bias is non-zero, RMSNorm weights lie
    in 0.5..1.5, the four ``alpha``s of an OmniShift in 0.19..0.31 (the module draws them from N(0, 1); their sum is the gain of the identity
    path) and ``gamma1`` / ``gamma2`` PER CHANNEL in 0.1..0.3: relu^2 and a dozen residual blocks grow fast, and the module's own
    initialisation (ones) would hide a per-channel indexing error.  The ``ps`` head of the reference's loader takes ``out_channels`` from
    ``inp_channels``: pass them equal for a checkpoint it is to load."""
    if upsampler not in FLEXNET_UPSAMPLERS:
        raise ValueError(f'unknown FlexNet upsampler {upsampler!r}')
    sd: OrderedDict = OrderedDict()
    g = float(np.sqrt(3.0))  # uniform(-g / sqrt(fan_in), ..): variance 1 / fan_in
    hidden = int(hidden_rate * dim)
    s = int(scale)

    def bias(name, co, gain=1.0):
        b = synth_tensor(name, (co,), 1, seed, 0.08 * g * gain)
        return b + 0.01 * gain * torch.where(b >= 0, 1.0, -1.0)  # never zero

    def conv(name, co, ci, k, groups=1, gain=1.0, with_bias=True):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci // groups, k, k), (ci // groups) * k * k, seed, g * gain)
        if with_bias:
            sd[f'{name}.bias'] = bias(f'{name}.bias', co, gain)

    def lin(name, co, ci, with_bias=True, gain=1.0):
        sd[f'{name}.weight'] = synth_tensor(f'{name}.weight', (co, ci), ci, seed, g * gain)
        if with_bias:
            sd[f'{name}.bias'] = bias(f'{name}.bias', co, gain)

    def rms(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 1, seed, 0.5)

    def omnishift(name, c):
        sd[f'{name}.alpha'] = 0.25 + synth_tensor(f'{name}.alpha', (4,), 1, seed, 0.06)
        for sub, ks in (('conv1x1', 1), ('conv3x3', 3), ('conv5x5', 5), ('conv5x5_reparam', 5)):
            conv(f'{name}.{sub}', c, c, ks, groups=c, with_bias=False)

    def convblock(name, ci, co):
        conv(f'{name}.block.0', co, ci, 3)
        conv(f'{name}.block.2', co, co, 3)
        conv(f'{name}.conv11', co, ci, 1, gain=0.5)

    sd['window_size'] = torch.tensor(8, dtype=torch.uint8)
    if upsampler == 'n+c':
        sd['scale_factor'] = torch.tensor(s, dtype=torch.uint8)
    convblock('short_cut', inp_channels, dim)
    conv('in_to_feat', dim, inp_channels, 3)
    for li, nb in enumerate(num_blocks):
        for bi in range(nb):
            b = f'pipeline.att.{li}.t_blocks.{bi}'
            sd[f'{b}.gamma1'] = 0.2 + synth_tensor(f'{b}.gamma1', (dim,), 1, seed, 0.1)
            sd[f'{b}.gamma2'] = 0.2 + synth_tensor(f'{b}.gamma2', (dim,), 1, seed, 0.1)
            rms(f'{b}.rn1', dim)
            rms(f'{b}.rn2', dim)
            lin(f'{b}.att.qkv', 3 * dim, dim, gain=1.5)  # (wider logits: a softmax over near-equal logits would hide a wrong key order)
            lin(f'{b}.att.proj', dim, dim)
            omnishift(f'{b}.att.omni_shift', dim)
            conv(f'{b}.att.get_v', dim, dim, 3, groups=dim)
            lin(f'{b}.ffn.key', hidden, dim, with_bias=False)
            omnishift(f'{b}.ffn.omni_shift', dim)
            if channel_norm:
                rms(f'{b}.ffn.key_norm', hidden)
            lin(f'{b}.ffn.receptance', dim, dim, with_bias=False)
            lin(f'{b}.ffn.value', dim, hidden, with_bias=False)
        convblock(f'pipeline.att.{li}.conv', 2 * dim, dim)
    if upsampler == 'n+c':
        conv('to_img.0', dim, 2 * dim, 3)
        i = 0
        if s & (s - 1) == 0:
            for _ in range(s.bit_length() - 1):
                conv(f'to_img.1.{i}', dim, dim, 3)
                i += 3
            conv(f'to_img.1.{i}', dim, dim, 3)
            i += 2
        elif s == 3:
            conv('to_img.1.0', dim, dim, 3)
            conv('to_img.1.3', dim, dim, 3)
            i = 5
        conv(f'to_img.1.{i}', out_channels, dim, 3, gain=0.5)
    elif upsampler == 'dys':
        h = torch.arange((-s + 1) / 2, (s - 1) / 2 + 1) / s
        sd['to_img.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
        conv('to_img.end_conv', out_channels, 2 * dim, 1, gain=0.5)
        conv('to_img.offset', 8 * s * s, 2 * dim, 1, gain=0.5)
        conv('to_img.scope', 8 * s * s, 2 * dim, 1, with_bias=False)
    else:
        conv('to_img.0', out_channels * s * s, 2 * dim, 3, gain=0.5)
    return sd


def smosr_state_dict(in_ch=3, out_ch=3, dim=48, scale=2, rep=False, n_mb=3, upsampler='pixelshuffledirect', upsampler_mid_dim=32, d_kernel=3,
                     head_gain=1.0, short_gain=1.0, seed=0):  # fmt: skip
    """Keys of the reference SMoSR module (archs/smosr/arch.py:419-459) in its registration order, which is the order the engine's module
    registers them in.  Every ``W`` is uniform * sqrt(3 / fan_in) * 0.5, ``D`` uniform in +-0.05 on top of the ``d_diag`` identity, ``mul``
    its initial value (3 in an SMB's body, 0.02 in a ConvNXC's ``sk``, 1 elsewhere) * (1 +- 0.1), so the fold matters; the two kinds of
    ``short`` are their 0 / 1 initial pattern plus uniform +-0.25 / sqrt(cin); every ``eval_conv.*`` is unrelated noise, which a correct
    implementation never reads.  ``head_gain`` scales the ``W`` of the head's last convolution (DySample's ``end_conv``) and ``short_gain``
    the global ``short``: the gains that bring ``|y|`` to order 1."""
    from ..archs.smosr.arch import SMoSR  # (not at import time: the architectures import this package's siblings)

    m = SMoSR(in_ch=in_ch, out_ch=out_ch, dim=dim, scale=scale, rep=rep, n_mb=n_mb, upsampler=upsampler, upsampler_mid_dim=upsampler_mid_dim, d_kernel=d_kernel)
    last = max(i for i, _, _, _ in m.head_convs) if m.head_convs else -1
    last_w = {f'upsampler.{m.dys_index}.end_conv.weight'} if m.dys_index is not None else {
        k for k in m._mul_init if k.startswith(f'upsampler.{last}.') and (not rep or '.conv.2.' in k or '.sk.' in k)}
    last_w = {k[: -len('mul')] + 'W' if k.endswith('.mul') else k for k in last_w}
    sd: OrderedDict = OrderedDict()
    for k, v in m.state_dict().items():
        shape, leaf = tuple(v.shape), k.rsplit('.', 1)[1]
        if k.endswith('MetaUpsample') or k.endswith('init_pos'):
            sd[k] = v.clone()
        elif '.eval_conv.' in k:
            sd[k] = synth_tensor(k, shape, 1, seed)
        elif leaf == 'mul':
            sd[k] = m._mul_init[k] * (1.0 + synth_tensor(k, shape, 1, seed, 0.1))
        elif leaf == 'W':
            sd[k] = synth_tensor(k, shape, shape[1] * shape[2], seed, 0.5 * 3**0.5 * (head_gain if k in last_w else 1.0))
        elif leaf == 'D':
            sd[k] = synth_tensor(k, shape, 1, seed, 0.05)
        elif leaf == 'd_diag':
            sd[k] = torch.eye(shape[1], dtype=torch.float32).reshape(1, shape[1], shape[1]).repeat(shape[0], 1, 1)
        elif k in ('short.weight', 'blocks_1.0.short.weight'):
            co, ci = shape[:2]
            w = torch.zeros(shape)
            if k == 'short.weight':  # channel c feeds outputs [c s^2, (c + 1) s^2)  (:437-442)
                for c in range(ci):
                    w[c * (co // ci) : (c + 1) * (co // ci), c] = 1.0
                w *= short_gain
            else:  # channel c feeds k or k + 1 consecutive outputs (:391-400)
                o = 0
                for c in range(ci):
                    n = co // ci + (1 if c < co % ci else 0)
                    w[o : o + n, c] = 1.0
                    o += n
            sd[k] = w + synth_tensor(k, shape, ci, seed, 0.25)
        elif k.endswith('.scope.weight'):
            sd[k] = synth_tensor(k, shape, shape[1], seed)
        elif k.endswith('.offset.weight') or k.endswith('.offset.bias'):
            sd[k] = synth_tensor(k, shape, shape[1] if len(shape) > 1 else m.mid_dim, seed, 0.5)
        elif k.endswith('.end_conv.weight'):
            sd[k] = synth_tensor(k, shape, shape[1] * shape[2] * shape[3], seed, head_gain)
        else:  # biases
            sd[k] = synth_tensor(k, shape, 16, seed, 0.25)
    return sd


GFISRV2_SAMPLE_MODS = MOSRV2_SAMPLE_MODS + ('transpose+conv', 'lda', 'pa_up')


def gfisrv2_state_dict(in_nc=3, out_nc=3, dim=48, scale=4, n_blocks=24, expansion_ratio=8 / 3, upsampler='pixelshuffledirect', mid_dim=32, seed=0):
    """Keys of the reference GFISRV2 module (archs/gfisrv2/arch.py:637-686) in its registration order: a block's ``gamma`` before its
    sub-modules, the four Inception branches under the attribute names that rotate with the block index, ``upscale.MetaUpsample`` before the
    head's layers (UniUpsampleV3 with a 3x3 DySample end convolution).  Scales, offsets, gammas and biases are all randomised; fc2 is drawn
    at half the default bound, which keeps the default depth (24 blocks) of order 1."""
    from ..archs.gfisrv2.arch import branch_order  # (not at import time: the architectures import this package's siblings)

    sd: OrderedDict = OrderedDict()
    hidden = int(expansion_ratio * dim)
    gc = int(dim * 0.125)
    cf = dim - 3 * gc

    def rms(name, c):
        sd[f'{name}.scale'] = 1.0 + synth_tensor(f'{name}.scale', (c, 1, 1), 16, seed)
        sd[f'{name}.offset'] = synth_tensor(f'{name}.offset', (c, 1, 1), 16, seed)

    _conv(sd, 'in_to_dim', dim, in_nc, 3, seed)
    for i in range(n_blocks):
        b = f'gfisr_body.{i}'
        sd[f'{b}.gamma'] = 1.0 + synth_tensor(f'{b}.gamma', (1, dim, 1, 1), 16, seed)
        rms(f'{b}.norm', dim)
        _conv(sd, f'{b}.fc1', 2 * hidden, dim, 3, seed)
        for name, kind in branch_order(i):
            c = f'{b}.conv.{name}'
            if kind is None:
                rms(f'{c}.rn', 2 * cf)
                rms(f'{c}.post_norm', cf)
                _conv(sd, f'{c}.fdc', 2 * cf, 2 * cf, 1, seed)
                _dwconv(sd, f'{c}.fpe', 2 * cf, 3, 3, seed)
            else:
                _dwconv(sd, c, gc, kind[0], kind[1], seed)
        _conv(sd, f'{b}.fc2', dim, hidden, 3, seed, scale=0.5)
    _conv(sd, f'gfisr_body.{n_blocks}', 2 * dim, dim, 3, seed)
    _conv(sd, f'gfisr_body.{n_blocks + 2}', dim, 2 * dim, 3, seed)
    _uni_upsample_v3(sd, 'gfisrv2_state_dict', upsampler, scale, dim, out_nc, mid_dim, seed)
    return sd


def _uni_upsample_v3(sd, who, up, s, dim, out_nc, mid_dim, seed):
    """UniUpsampleV3 with a 3x3 DySample end convolution under ``upscale``, as GFISRv2 and FIGSR register it."""
    meta = torch.tensor([3, GFISRV2_SAMPLE_MODS.index(up), s, dim, out_nc, mid_dim, 4], dtype=torch.uint8)
    if s != 1 and up == 'dysample':
        sd['upscale.MetaUpsample'] = meta
        i, dys_dim = 0, dim
        if mid_dim != dim:
            _conv(sd, 'upscale.0', mid_dim, dim, 3, seed)
            i, dys_dim = 2, mid_dim
        oc = 8 * s * s
        h = torch.arange((-s + 1) / 2, (s - 1) / 2 + 1) / s  # (DySample's own buffer: before its sub-modules)
        sd[f'upscale.{i}.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
        _conv(sd, f'upscale.{i}.end_conv', out_nc, dys_dim, 3, seed)
        _conv(sd, f'upscale.{i}.offset', oc, dys_dim, 1, seed, scale=0.5)
        _conv(sd, f'upscale.{i}.scope', oc, dys_dim, 1, seed, bias=False)
    elif s == 1 or up in MOSRV2_SAMPLE_MODS:
        _uni_upsample(sd, 'upscale', 'conv' if s == 1 else up, s, dim, out_nc, mid_dim, seed, version=3)
        sd['upscale.MetaUpsample'] = meta  # (the same place in the order; at scale 1 every mode is the one convolution)
    else:
        raise ValueError(f'{who}: the {up!r} head is not synthesised')


def figsr_state_dict(in_nc=3, out_nc=3, dim=48, scale=4, n_blocks=24, expansion_ratio=8 / 3, upsampler='pixelshuffledirect', mid_dim=32, gc=8,
                     square_kernel_size=13, band_kernel_size=17, shift=(0.5, 0.5, 0.5), scale_norm=(1 / 6, 1 / 6, 1 / 6), halves=None, seed=0):  # fmt: skip
    """Keys of the reference FIGSR module (archs/figsr/arch.py:624-664) in its registration order: the module's own ``shift`` and
    ``scale_norm`` first, every RMSNorm with its ``eps`` and ``rms`` parameters (at the reference's values), the two halves (``halves``:
    their block counts where they shall NOT be the reference's (n // 2, n - n // 2)), the 3x3 convolution behind the second half,
    ``cat_to_dim``, then ``upscale.MetaUpsample`` before the head's layers.  Scales, offsets and biases are all randomised; fc2 is drawn at
    half the default bound, which keeps the default depth (24 blocks) of order 1."""
    sd: OrderedDict = OrderedDict()
    hidden = int(expansion_ratio * dim) // 8 * 8
    cf = dim - 3 * gc

    def rms(name, c):
        sd[f'{name}.scale'] = 1.0 + synth_tensor(f'{name}.scale', (c,), 16, seed)
        sd[f'{name}.offset'] = synth_tensor(f'{name}.offset', (c,), 16, seed)
        sd[f'{name}.eps'] = torch.ones(1) * 1e-6
        sd[f'{name}.rms'] = torch.ones(1) * (c**-0.5)

    sd['shift'] = torch.tensor(shift, dtype=torch.float32).reshape(1, 3, 1, 1)
    sd['scale_norm'] = torch.tensor(scale_norm, dtype=torch.float32).reshape(1, 3, 1, 1)
    _conv(sd, 'in_to_dim', dim, in_nc, 3, seed)
    n1, n2 = (n_blocks // 2, n_blocks - n_blocks // 2) if halves is None else halves
    for b in [f'gfisr_body_half.{i}' for i in range(n1)] + [f'gfisr_body_half_2.{i}' for i in range(n2)]:
        rms(f'{b}.norm', dim)
        _conv(sd, f'{b}.fc1', 2 * hidden, dim, 3, seed)
        c = f'{b}.conv.fu'
        rms(f'{c}.rn', 2 * cf)
        rms(f'{c}.post_norm', cf)
        _conv(sd, f'{c}.fdc', 2 * cf, 2 * cf, 1, seed)
        _dwconv(sd, f'{c}.fpe', 2 * cf, 3, 3, seed)
        _conv(sd, f'{b}.conv.convhw', gc, gc, square_kernel_size, seed)
        for name, kh, kw in (('convw', 1, band_kernel_size), ('convh', band_kernel_size, 1)):
            sd[f'{b}.conv.{name}.weight'] = synth_tensor(f'{b}.conv.{name}.weight', (gc, gc, kh, kw), gc * kh * kw, seed)
            sd[f'{b}.conv.{name}.bias'] = synth_tensor(f'{b}.conv.{name}.bias', (gc,), gc * kh * kw, seed)
        _conv(sd, f'{b}.fc2', dim, hidden, 3, seed, scale=0.5)
    _conv(sd, f'gfisr_body_half_2.{n2}', dim, dim, 3, seed)
    _conv(sd, 'cat_to_dim', dim, 3 * dim, 1, seed)
    _uni_upsample_v3(sd, 'figsr_state_dict', upsampler, scale, dim, out_nc, mid_dim, seed)
    return sd


def lawfft_state_dict(in_ch=3, dim=60, local=15, scale=4, n_rblock=4, n_mblock=6, t_mid_factor=1.0, window_size=8, mlp_factor=2.66,
                      upsampler='pixelshuffledirect', mid_dim=48, unshuffle_mod=False, to_hidden_rows=None, seed=0):  # fmt: skip
    """Keys and dtypes of the reference LAWFFT module (archs/lawfft/arch.py:380-416) in its registration order: the uint8 ``window_size``
    buffer first, ``upscale.MetaUpsample`` before the head's layers.  ``local`` is the local width itself (the reference derives it from a
    float ``split``); the FSAS width is ``int(global * t_mid_factor)`` and ``to_hidden`` has ``int(global * 3 * t_mid_factor)`` rows, as the
    reference computes them (``to_hidden_rows`` overrides the latter).  The kernel generators' first layer is drawn twice as wide as
    the default bound, with a bias of the pooled input's order: some of its ReLUs are active and some are not; the second layer's bias is
    bounded by 1 / k^2, so a generated kernel's taps sum to order 1.  The 1x1 convolutions behind a residual are drawn at half the
    default bound and the generators' second layers at an eighth of it -- a generated kernel scales with the pooled mean of its own input,
    so a larger gain squares the stream from group to group on large images --, which keeps the default depth (24 blocks) of order 1 from
    9 x 11 to 512 x 512."""
    sd: OrderedDict = OrderedDict()
    glob = dim - local
    fsas, rows = int(glob * t_mid_factor), int(glob * 3 * t_mid_factor) if to_hidden_rows is None else to_hidden_rows
    hid = int(dim * mlp_factor)
    sd['window_size'] = torch.tensor(window_size, dtype=torch.uint8)
    s_int = scale
    if unshuffle_mod and scale < 3:
        u = 4 // scale
        _conv(sd, 'in_to_dim.1', dim, in_ch * u * u, 3, seed)
        s_int = 4
    else:
        _conv(sd, 'in_to_dim', dim, in_ch, 3, seed)

    def norm(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), 16, seed)

    def gen(name, c, k):
        _conv(sd, f'{name}.kernel_gen.1', c, c, 1, seed, scale=2.0)
        sd[f'{name}.kernel_gen.1.bias'] = synth_tensor(f'{name}.kernel_gen.1.bias', (c,), 4, seed)
        _conv(sd, f'{name}.kernel_gen.3', c * k * k, c, 1, seed, scale=0.125)
        sd[f'{name}.kernel_gen.3.bias'] = synth_tensor(f'{name}.kernel_gen.3.bias', (c * k * k,), k**4, seed)

    for r in range(n_rblock):
        for i in range(n_mblock):
            b = f'body.{r}.residual.{i}'
            t, a, c = f'{b}.token_mix', f'{b}.token_mix.1.att', f'{b}.channel_mix1'
            norm(f'{t}.0', dim)
            gen(f'{t}.1.local.0', local, 3)
            gen(f'{t}.1.local.1', local, 5)
            _conv(sd, f'{a}.to_hidden', rows, glob, 1, seed)
            _dwconv(sd, f'{a}.to_hidden_dw', rows, 3, 3, seed)
            _conv(sd, f'{a}.project_out', glob, fsas, 1, seed)
            norm(f'{a}.norm', fsas)
            _conv(sd, f'{t}.1.last', dim, dim, 1, seed, scale=0.5)
            norm(f'{c}.0', dim)
            _conv(sd, f'{c}.1.project_in', 2 * hid, dim, 1, seed)
            _dwconv(sd, f'{c}.1.dwconv', 2 * hid, 3, 3, seed)
            _conv(sd, f'{c}.1.project_out', dim, hid, 1, seed, scale=0.5)
        gen(f'body.{r}.residual.{n_mblock}', dim, 3)
    _uni_upsample(sd, 'upscale', 'conv' if s_int == 1 else upsampler, s_int, dim, in_ch, mid_dim, seed, version=2)
    sd['upscale.MetaUpsample'] = torch.tensor([2, MOSRV2_SAMPLE_MODS.index(upsampler), s_int, dim, in_ch, mid_dim, 4], dtype=torch.uint8)
    if upsampler == 'dysample' and s_int != 1 and mid_dim != dim:  # UniUpsample (version 2): a mid_dim convolution in front of DySample
        for k in [k for k in sd if k.startswith('upscale.0.')]:
            del sd[k]
        _conv(sd, 'upscale.0', mid_dim, dim, 3, seed)
        oc = 8 * s_int * s_int
        h = torch.arange((-s_int + 1) / 2, (s_int - 1) / 2 + 1) / s_int
        sd['upscale.2.init_pos'] = torch.stack(torch.meshgrid([h, h], indexing='ij')).transpose(1, 2).repeat(1, 4, 1).reshape(1, -1, 1, 1)
        _conv(sd, 'upscale.2.end_conv', in_ch, mid_dim, 1, seed)
        _conv(sd, 'upscale.2.offset', oc, mid_dim, 1, seed, scale=0.5)
        _conv(sd, 'upscale.2.scope', oc, mid_dim, 1, seed, bias=False)
    return sd


GFISR_SLOTS = ('pconv', 'dwconv_hw', 'dwconv_w', 'dwconv_h', 'fsas')  # InceptionDWConv2d's attribute names of GFISR (v1), in channel order
GFISR_KINDS = ('identity', (3, 3), (1, 11), (11, 1), 'fourier')  # its five modules before rotation


def gfisr_state_dict(in_nc=3, out_nc=3, dim=48, scale=4, n_blocks=24, expansion_ratio=8 / 3, upsampler='pixelshuffledirect', mid_dim=32,
                     fft_mode=True, pixel_unshuffle=False, seed=0):  # fmt: skip
    """Keys of the reference GFISR module (archs/gfisr/arch.py:594-629) in its registration order: a block's ``gamma`` before its
    sub-modules, the five Inception modules under the attribute names that rotate with the block index (the identity registers nothing; the
    FourierUnit registers ``ln``, ``fdc``, the 1x1 convolution ``weight.0`` in front of its one-channel softmax, ``fpe``),
    ``dim_to_out.MetaUpsample`` before the head's layers (UniUpsampleV3 with a 3x3 DySample end convolution).  ``pixel_unshuffle`` with
    scale 1 or 2 gives ``in_to_dim.1`` over ``in_nc * (4 // scale) ** 2`` channels and a head of scale 4, as the reference module builds
    them.  Norms, gammas and biases are all randomised; fc2 is drawn at half the default bound, which keeps the default depth (24 blocks)
    of order 1."""
    sd: OrderedDict = OrderedDict()
    hidden = int(expansion_ratio * dim)
    gc = int(dim / 8)
    head_scale = scale

    def norm(name, c):
        sd[f'{name}.weight'] = 1.0 + synth_tensor(f'{name}.weight', (c,), 16, seed)
        sd[f'{name}.bias'] = synth_tensor(f'{name}.bias', (c,), 16, seed)

    if pixel_unshuffle and scale in (1, 2):
        down = 4 // scale
        _conv(sd, 'in_to_dim.1', dim, in_nc * down * down, 3, seed)
        head_scale = 4
    else:
        _conv(sd, 'in_to_dim', dim, in_nc, 3, seed)
    for i in range(n_blocks):
        b = f'net.{i}'
        sd[f'{b}.gamma'] = 1.0 + synth_tensor(f'{b}.gamma', (1, dim, 1, 1), 16, seed)
        norm(f'{b}.norm', dim)
        _conv(sd, f'{b}.fc1', 2 * hidden, dim, 3, seed)
        for t, name in enumerate(GFISR_SLOTS):
            kind, c = GFISR_KINDS[(i + t) % 5], f'{b}.conv.{name}'
            if kind == 'fourier' and fft_mode:
                norm(f'{c}.ln', 2 * gc)
                _conv(sd, f'{c}.fdc', 2 * gc, 2 * gc, 1, seed)
                _conv(sd, f'{c}.weight.0', 1, 2 * gc, 1, seed)
                _dwconv(sd, f'{c}.fpe', 2 * gc, 3, 3, seed)
            elif isinstance(kind, tuple):
                _dwconv(sd, c, gc, kind[0], kind[1], seed)
        _conv(sd, f'{b}.fc2', dim, hidden, 3, seed, scale=0.5)
    head: OrderedDict = OrderedDict()
    _uni_upsample_v3(head, 'gfisr_state_dict', upsampler, head_scale, dim, out_nc, mid_dim, seed)
    for k, v in head.items():
        sd['dim_to_out.' + k[len('upscale.') :]] = v
    return sd


def gaterv3_state_dict(in_ch=3, dim=32, enc_blocks=(2, 2, 4, 8), dec_blocks=(2, 2, 2, 2), num_latent=12, scale=1, upsample='pixelshuffle',
                       upsample_mid_dim=32, attention=False, span_blocks=4, end_kernel=3, with_gamma=True, seed=0):  # fmt: skip
    """Keys of the reference GateRV3 module (archs/gaterv3/arch.py:705-802) in the order of its ``state_dict()``: a module's own parameters
    before its children's (``gamma`` first, ``gamma0`` / ``gamma1`` at the head of a MetaGated, ``temperature`` at the head of an Attention),
    the SPABs' Conv3XC without biases, ``dim_to_in.MetaUpsample`` before the head's layers and DySample's ``init_pos`` before its
    convolutions; at scale 1 ``dim_to_in`` is one plain convolution and there is no MetaUpsample buffer.  ``with_gamma=False`` leaves
    ``gamma`` out (the loader then keeps the module's ones).
    Matrices and filters are uniform with variance 1 / fan_in, so that a layer has roughly unit gain; norm scales lie in 0.5..1.5, offsets
    in +-0.1, biases in +-0.09, ``gamma0`` / ``gamma1`` in +-0.5 per channel (both signs; a stream grows by about a tenth of its variance
    per block, and every block renormalises), the temperatures in -0.5..2.5 per head, the last convolution at a tenth of the bound: the
    output stays of order 1 through four levels (N(0, 0.1) weights throughout give |y| of about 400 there)."""
    from ..archs.gaterv3.arch import trunk_shapes
    from ..engine.uniupsample import Head

    sd: OrderedDict = OrderedDict()
    g = float(np.sqrt(3.0))

    def fill(name, shape, gain=1.0):
        leaf = name.rsplit('.', 1)[-1]
        if name == 'gamma':
            sd[name] = 1.0 + synth_tensor(name, shape, 1, seed, 0.3)
        elif leaf in ('gamma0', 'gamma1'):
            sd[name] = synth_tensor(name, shape, 1, seed, 0.5)
        elif leaf == 'scale' and len(shape) == 1:
            sd[name] = 1.0 + synth_tensor(name, shape, 1, seed, 0.5)
        elif leaf == 'offset':
            sd[name] = synth_tensor(name, shape, 1, seed, 0.1)
        elif leaf == 'temperature':
            sd[name] = 1.0 + synth_tensor(name, shape, 1, seed, 1.5)
        elif leaf == 'bias':
            sd[name] = synth_tensor(name, shape, 1, seed, 0.05 * g * gain)
        else:
            sd[name] = synth_tensor(name, shape, int(np.prod(shape[1:])), seed, g * gain)

    for name, shape in trunk_shapes(in_ch, dim, tuple(enc_blocks), tuple(dec_blocks), num_latent, attention, span_blocks).items():
        if name == 'gamma' and not with_gamma:
            continue
        fill(name, shape)
    if scale == 1:
        fill('dim_to_in.weight', (in_ch, dim, 3, 3), 0.1)
        fill('dim_to_in.bias', (in_ch,), 0.1)
        return sd
    head = Head('dim_to_in', upsample, scale, dim, in_ch, upsample_mid_dim, end_kernel=end_kernel, version=3)
    shapes, buffers = {}, {}
    head.shapes(shapes, buffers)
    sd['dim_to_in.MetaUpsample'] = buffers['dim_to_in.MetaUpsample']
    last = f'dim_to_in.{head.layers[-1][0]}.' if head.dys_index is None else '.end_conv.'
    pos = [k for k in buffers if k.endswith('init_pos')]
    dys = f'dim_to_in.{head.dys_index}.' if head.dys_index is not None else None
    for name, shape in shapes.items():
        if dys is not None and name.startswith(dys) and pos:
            key = pos.pop()
            sd[key] = buffers[key]
        fill(name, shape, 0.1 if last in name else (0.5 if '.offset.' in name else 1.0))
    return sd


def gaterv2_state_dict(in_ch=3, dim=48, enc_blocks=(2, 2, 4, 6), dec_blocks=(2, 2, 2, 2), num_latent=10, scale=1, upsample='pixelshuffledirect',
                       upsample_mid_dim=32, seed=0):  # fmt: skip
    """Keys of the reference GateRV2 module (archs/gaterv2/arch.py:394-470) in the order of its ``state_dict()``: the trunk, then at scale 1
    the plain ``dim_to_in`` convolution, above it ``short_to_dim`` (the ConvBlock: block.0, block.2, conv11) and ``upsample`` (UniUpsample
    v1: the MetaUpsample buffer first, DySample's ``init_pos`` before its convolutions).
    The value distributions are ``gaterv3_state_dict``'s: matrices and filters uniform with variance 1 / fan_in, norm scales in 0.5..1.5,
    offsets in +-0.1, biases in +-0.09 (the q / k / v biases included, so that no token's query or key vector is zero), ``gamma0`` /
    ``gamma1`` in +-0.5 per channel, the last convolution at a tenth of the bound."""
    from ..archs.gaterv2.arch import trunk_shapes
    from ..engine.uniupsample import Head

    sd: OrderedDict = OrderedDict()
    g = float(np.sqrt(3.0))

    def fill(name, shape, gain=1.0):
        leaf = name.rsplit('.', 1)[-1]
        if leaf in ('gamma0', 'gamma1'):
            sd[name] = synth_tensor(name, shape, 1, seed, 0.5)
        elif leaf == 'scale' and len(shape) == 1:
            sd[name] = 1.0 + synth_tensor(name, shape, 1, seed, 0.5)
        elif leaf == 'offset':
            sd[name] = synth_tensor(name, shape, 1, seed, 0.1)
        elif leaf == 'bias':
            sd[name] = synth_tensor(name, shape, 1, seed, 0.05 * g * gain)
        else:
            sd[name] = synth_tensor(name, shape, int(np.prod(shape[1:])), seed, g * gain)

    for name, shape in trunk_shapes(in_ch, dim, tuple(enc_blocks), tuple(dec_blocks), num_latent).items():
        fill(name, shape)
    if scale == 1:
        fill('dim_to_in.weight', (in_ch, dim, 3, 3), 0.1)
        fill('dim_to_in.bias', (in_ch,), 0.1)
        return sd
    for name, co, ci, k in (('short_to_dim.block.0', dim, in_ch, 3), ('short_to_dim.block.2', dim, dim, 3), ('short_to_dim.conv11', dim, in_ch, 1)):
        fill(f'{name}.weight', (co, ci, k, k))
        fill(f'{name}.bias', (co,))
    head = Head('upsample', upsample, scale, dim, in_ch, dim if upsample == 'dysample' else upsample_mid_dim, version=1, meta_mid_dim=upsample_mid_dim)
    shapes, buffers = {}, {}
    head.shapes(shapes, buffers)
    sd['upsample.MetaUpsample'] = buffers['upsample.MetaUpsample']
    last = f'upsample.{head.layers[-1][0]}.' if head.dys_index is None else '.end_conv.'
    pos = [k for k in buffers if k.endswith('init_pos')]
    for name, shape in shapes.items():
        if pos and head.dys_index is not None:
            key = pos.pop()
            sd[key] = buffers[key]
        fill(name, shape, 0.1 if last in name else (0.5 if '.offset.' in name else 1.0))
    return sd
