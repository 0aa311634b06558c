"""Plain-PyTorch restatement (in the dtype of the input: fp64 for a high-precision reference, and then the transforms run in fp64 too) of
the LAWFFT forward from a state dict (CPU), written from the layer description in resselt_amd/archs/lawfft.  The correlation of FSAS exists
twice: ``corr_fft`` (rfft2, product, irfft2 with torch's default 'backward' normalisation) and ``corr_direct``, the circular convolution
``corr[y, x] = sum_{u, v} q[u, v] k[(y - u) mod P, (x - v) mod Q]`` summed as written, which checks the FFT form against the definition."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from mosr_oracle import _conv, _dw, _head, _layer_norm

MODES = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')
WINDOW = 8


def corr_fft(q, k):
    """The circular convolution of the last two dimensions through the real FFT."""
    return torch.fft.irfft2(torch.fft.rfft2(q) * torch.fft.rfft2(k), s=q.shape[-2:])


def corr_direct(q, k):
    """The same sum, term by term: every (u, v) shift of k weighted by q[u, v]."""
    out = torch.zeros_like(q)
    for u in range(q.shape[-2]):
        for v in range(q.shape[-1]):
            out = out + q[..., u : u + 1, v : v + 1] * torch.roll(k, shifts=(u, v), dims=(-2, -1))
    return out


def to_patches(x, p=WINDOW):
    b, c, h, w = x.shape
    return x.view(b, c, h // p, p, w // p, p).permute(0, 1, 2, 4, 3, 5)


def from_patches(x):
    b, c, nh, nw, p, _ = x.shape
    return x.permute(0, 1, 2, 4, 3, 5).reshape(b, c, nh * p, nw * p)


def dynamic_local(sd, p, x):
    """One k x k kernel per sample and channel, generated from the sample's pooled channels; zero padding, no bias."""
    b, c, h, w = x.shape
    m = x.mean((2, 3), keepdim=True)
    hid = F.relu(F.conv2d(m, sd[f'{p}.kernel_gen.1.weight'], sd[f'{p}.kernel_gen.1.bias']))
    kernels = F.conv2d(hid, sd[f'{p}.kernel_gen.3.weight'], sd[f'{p}.kernel_gen.3.bias'])
    k = int(round((kernels.shape[1] // c) ** 0.5))
    return F.conv2d(x.reshape(1, b * c, h, w), kernels.reshape(b * c, 1, k, k), padding=k // 2, groups=b * c).reshape(b, c, h, w)


def fsas(sd, p, x, windowed, corr=corr_fft):
    q, k, v = _dw(F.conv2d(x, sd[f'{p}.to_hidden.weight'], sd[f'{p}.to_hidden.bias']), sd[f'{p}.to_hidden_dw.weight'], sd[f'{p}.to_hidden_dw.bias']).chunk(3, dim=1)
    out = from_patches(corr(to_patches(q), to_patches(k))) if windowed else corr(q, k)
    out = _layer_norm(out, sd[f'{p}.norm.weight'], sd[f'{p}.norm.bias'])
    return F.conv2d(v * out, sd[f'{p}.project_out.weight'], sd[f'{p}.project_out.bias'])


def meta_block(sd, b, x, windowed, corr=corr_fft):
    t, c = f'{b}.token_mix', f'{b}.channel_mix1'
    local = sd[f'{t}.1.local.0.kernel_gen.1.bias'].shape[0]
    n = _layer_norm(x, sd[f'{t}.0.weight'], sd[f'{t}.0.bias'])
    x1 = dynamic_local(sd, f'{t}.1.local.1', dynamic_local(sd, f'{t}.1.local.0', n[:, :local]))
    x2 = fsas(sd, f'{t}.1.att', n[:, local:], windowed, corr)
    x = x + F.conv2d(torch.cat([x1, x2], 1), sd[f'{t}.1.last.weight'], sd[f'{t}.1.last.bias'])
    n = _layer_norm(x, sd[f'{c}.0.weight'], sd[f'{c}.0.bias'])
    g1, g2 = _dw(_conv(sd, f'{c}.1.project_in', n), sd[f'{c}.1.dwconv.weight'], sd[f'{c}.1.dwconv.bias']).chunk(2, dim=1)
    return x + _conv(sd, f'{c}.1.project_out', F.gelu(g1) * g2)


def lawfft_forward(sd, x, corr=corr_fft):
    """``sd``: a LAWFFT state dict (``upscale.MetaUpsample`` names the head and the scale); ``x`` [N, C, H, W]."""
    _, index, scale, _, _, mid_dim = (int(v) for v in sd['upscale.MetaUpsample'][:6])
    sd = {k: v.to(x.dtype) for k, v in sd.items() if k not in ('window_size', 'upscale.MetaUpsample')}
    h, w = x.shape[-2:]
    t = F.pad(x, (0, (WINDOW - w % WINDOW) % WINDOW, 0, (WINDOW - h % WINDOW) % WINDOW), mode='reflect')
    t0 = t = _conv(sd, 'in_to_dim', t)
    r = 0
    while f'body.{r}.residual.0.token_mix.0.weight' in sd:
        g, i = t, 0
        while f'body.{r}.residual.{i}.token_mix.0.weight' in sd:
            g = meta_block(sd, f'body.{r}.residual.{i}', g, bool(i % 2), corr)
            i += 1
        t = dynamic_local(sd, f'body.{r}.residual.{i}', g) + t
        r += 1
    head = {k.replace('upscale.', 'to_img.', 1): v for k, v in sd.items() if k.startswith('upscale.')}
    y = _head(head, t + t0, MODES[index], scale, mid_dim)
    return y[:, :, : h * scale, : w * scale]
