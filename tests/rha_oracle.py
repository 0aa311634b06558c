"""A functional restatement of RHA's eval-mode forward in plain torch, written from the math (not from the reference's module code): the
reflect pad to a multiple of max(down) * window, to_feat, the groups of gated blocks with HybridAttention, the UniUpsample head and the crop.
It runs in the dtype of ``x`` (f32 or f64).  OmniShift is always rebuilt from its training parameters: the stored ``conv5x5_reparam`` pair
is never read, as in the reference's ``.eval()``."""

import math

import torch
import torch.nn.functional as F

SAMPLE_MODS = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')
HEADS = 8


def hyper(sd):
    dim, in_ch = sd['to_feat.weight'].shape[:2]
    groups = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('body.'))
    res = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('body.0.body.')) - 2
    _, idx, scale, _, out_ch, mid, _ = (int(v) for v in sd['to_img.MetaUpsample'])
    return dict(dim=dim, in_ch=in_ch, groups=groups, res=res, down=[int(sd[f'body.{g}.down_sample']) for g in range(groups)],
                hidden=sd['body.0.body.0.fc1.weight'].shape[0] // 2, head=SAMPLE_MODS[idx], scale=scale, out_ch=out_ch, mid=mid,
                ws=math.isqrt(sd['body.0.body.0.conv.att.2.positional_encoding'].shape[1]))  # fmt: skip


def layernorm(x, w, b):
    u = x.mean(1, keepdim=True)
    s = ((x - u) ** 2).mean(1, keepdim=True)
    return (x - u) / torch.sqrt(s + 1e-6) * w[None, :, None, None] + b[None, :, None, None]


def omnishift(sd, key, x):
    """alpha1 x + alpha2 dw1(x) + alpha3 dw3(x) + alpha4 dw5(x), as one 5x5 depthwise kernel."""
    t = x.dtype
    c = x.shape[1]
    a = [sd[f'{key}.alpha{k}'].to(t).reshape(c, 1, 1, 1) for k in (1, 2, 3, 4)]
    ident = torch.zeros((c, 1, 5, 5), dtype=t)
    ident[:, :, 2, 2] = 1
    w = a[0] * ident + a[1] * F.pad(sd[f'{key}.conv1x1.weight'].to(t), (2, 2, 2, 2)) + a[2] * F.pad(sd[f'{key}.conv3x3.weight'].to(t), (1, 1, 1, 1))
    w = w + a[3] * sd[f'{key}.conv5x5.weight'].to(t)
    b = a[1].flatten() * sd[f'{key}.conv1x1.bias'].to(t) + a[2].flatten() * sd[f'{key}.conv3x3.bias'].to(t) + a[3].flatten() * sd[f'{key}.conv5x5.bias'].to(t)
    return F.conv2d(x, w, b, padding=2, groups=c)


def window_attention(sd, key, x, ws):
    """FocusedLinearAttention on every ws x ws window of x [B, C, H, W]."""
    t = x.dtype
    B, C, H, W = x.shape
    d, N = C // HEADS, ws * ws
    win = x.reshape(B, C, H // ws, ws, W // ws, ws).permute(0, 2, 4, 3, 5, 1).reshape(-1, N, C)
    qkv = win @ sd[f'{key}.qkv.weight'].to(t).T + sd[f'{key}.qkv.bias'].to(t)
    q, k, v = qkv[..., :C], qkv[..., C : 2 * C], qkv[..., 2 * C :]
    k = k + sd[f'{key}.positional_encoding'].to(t).reshape(1, N, C)
    sp = F.softplus(sd[f'{key}.scale'].to(t)).reshape(1, 1, C)

    def focus(u):
        u = (u.clamp(min=0) + 1e-6) / sp
        n1 = u.norm(dim=-1, keepdim=True)
        u3 = u**3
        return u3 / u3.norm(dim=-1, keepdim=True) * n1

    q, k = focus(q), focus(k)
    nw = win.shape[0]
    qh, kh, vh = (u.reshape(nw, N, HEADS, d).transpose(1, 2) for u in (q, k, v))  # [nw, heads, N, d]
    z = 1.0 / ((qh * kh.mean(dim=2, keepdim=True)).sum(-1, keepdim=True) + 1e-6)
    kv = kh.transpose(-2, -1) @ vh / N
    out = (qh @ kv * z).transpose(1, 2).reshape(nw, N, C)
    vm = vh.reshape(nw * HEADS, ws, ws, d).permute(0, 3, 1, 2)  # every head of every window is an image of d channels
    dw = F.conv2d(vm, sd[f'{key}.dwc.weight'].to(t), sd[f'{key}.dwc.bias'].to(t), padding=2, groups=d)
    out = out + dw.reshape(nw, HEADS, d, N).permute(0, 3, 1, 2).reshape(nw, N, C)
    out = out @ sd[f'{key}.proj.weight'].to(t).T + sd[f'{key}.proj.bias'].to(t)
    return out.reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


def hybrid_attention(sd, key, c, down, shift, ws):
    x1, x2 = c.chunk(2, dim=1)
    x1 = omnishift(sd, f'{key}.conv', x1)
    if down > 1:
        x2 = F.max_pool2d(x2, down, down)
    if shift:
        x2 = torch.roll(x2, (-shift, -shift), (2, 3))
    x2 = window_attention(sd, f'{key}.att.2', x2, ws)
    if shift:
        x2 = torch.roll(x2, (shift, shift), (2, 3))
    if down > 1:
        x2 = F.interpolate(x2, scale_factor=down, mode='bilinear', align_corners=False)
    t = c.dtype
    a = F.mish(F.conv2d(torch.cat((x1, x2), 1), sd[f'{key}.aggr.0.weight'].to(t), sd[f'{key}.aggr.0.bias'].to(t)))
    return a * c


def block(sd, key, x, dim, hidden, down, shift, ws):
    t = x.dtype
    y = layernorm(x, sd[f'{key}.norm.weight'].to(t), sd[f'{key}.norm.bias'].to(t))
    y = F.conv2d(y, sd[f'{key}.fc1.weight'].to(t), sd[f'{key}.fc1.bias'].to(t), padding=1)
    g, i, c = torch.split(y, [hidden, hidden - dim, dim], dim=1)
    c = hybrid_attention(sd, f'{key}.conv', c, down, shift, ws)
    y = F.conv2d(F.mish(g) * torch.cat((i, c), 1), sd[f'{key}.fc2.weight'].to(t), sd[f'{key}.fc2.bias'].to(t), padding=1)
    return F.mish(y) + x


def dysample(sd, key, x, s, groups=4):
    t = x.dtype
    off = F.conv2d(x, sd[f'{key}.offset.weight'].to(t), sd[f'{key}.offset.bias'].to(t)) * torch.sigmoid(F.conv2d(x, sd[f'{key}.scope.weight'].to(t))) * 0.5
    off = off + sd[f'{key}.init_pos'].to(t)
    B, _, H, W = off.shape
    off = off.view(B, 2, -1, H, W)
    cw, ch = torch.arange(W, dtype=t) + 0.5, torch.arange(H, dtype=t) + 0.5
    coords = torch.stack(torch.meshgrid([cw, ch], indexing='ij')).transpose(1, 2).unsqueeze(1).unsqueeze(0)
    coords = 2 * (coords + off) / torch.tensor([W, H], dtype=t).view(1, 2, 1, 1, 1) - 1
    coords = F.pixel_shuffle(coords.reshape(B, -1, H, W), s).view(B, 2, -1, s * H, s * W).permute(0, 2, 3, 4, 1).contiguous().flatten(0, 1)
    out = F.grid_sample(x.reshape(B * groups, -1, H, W), coords, mode='bilinear', align_corners=False, padding_mode='border').view(B, -1, s * H, s * W)
    return F.conv2d(out, sd[f'{key}.end_conv.weight'].to(t), sd[f'{key}.end_conv.bias'].to(t))


def head(sd, x, hp):
    t = x.dtype
    cv = lambda i, v: F.conv2d(v, sd[f'to_img.{i}.weight'].to(t), sd[f'to_img.{i}.bias'].to(t), padding=1)  # noqa: E731
    up, s = hp['head'], hp['scale']
    if s == 1 or up == 'conv':
        return cv(0, x)
    if up == 'pixelshuffledirect':
        return F.pixel_shuffle(cv(0, x), s)
    pow2 = s & (s - 1) == 0
    if up == 'pixelshuffle':
        x = F.leaky_relu(cv(0, x), 0.01)
        i = 2
        for r in [2] * (s.bit_length() - 1) if pow2 else [3]:
            x = F.pixel_shuffle(cv(i, x), r)
            i += 2
        return cv(i, x)
    if up == 'nearest+conv':
        i = 0
        for r in [2] * (s.bit_length() - 1) if pow2 else [3]:
            x = F.leaky_relu(F.interpolate(cv(i, x), scale_factor=r, mode='nearest'), 0.2)
            i += 3
        return cv(i + 2, F.leaky_relu(cv(i, x), 0.2))
    i = 0
    if hp['mid'] != hp['dim']:
        x = F.leaky_relu(cv(0, x), 0.01)
        i = 2
    return dysample(sd, f'to_img.{i}', x, s)


def rha_forward(sd, x):
    hp = hyper(sd)
    t = x.dtype
    dim, ws = hp['dim'], hp['ws']
    _, _, h, w = x.shape
    pad = max(hp['down']) * ws
    x = F.pad(x, (0, (pad - w % pad) % pad, 0, (pad - h % pad) % pad), 'reflect')
    x = F.conv2d(x, sd['to_feat.weight'].to(t), sd['to_feat.bias'].to(t), padding=1)
    top = x
    for g in range(hp['groups']):
        gin = x
        for i in range(hp['res']):
            x = block(sd, f'body.{g}.body.{i}', x, dim, hp['hidden'], hp['down'][g], 0 if i % 2 == 0 else ws // 2, ws)
        x = omnishift(sd, f'body.{g}.body.{hp["res"]}', x)
        k = f'body.{g}.body.{hp["res"] + 1}'
        x = F.conv2d(x, sd[f'{k}.weight'].to(t), sd[f'{k}.bias'].to(t)) + gin
    x = x + top
    return head(sd, x, hp)[:, :, : h * hp['scale'], : w * hp['scale']]
