"""Plan-side plumbing of the dense real 2-D DFT (``rsa_gfisr_dft``; GFISR, GFISRv2, FIGSR, LAWFFT) and of the FourierUnit GFISRv2 and FIGSR share.

``dft_workspace`` builds what every transform of one size needs, once per plan: the scratch buffer and the four 'ortho' tables
(``lib_gfisr.dft_tables``, which depend on (H, W) alone).  ``emit_dft`` is one transform of ``channels`` channels between planes and an f32
spectral map [real | imag].  ``pack_fourier_unit`` / ``emit_fourier_unit`` are the v2 FourierUnit: rfft2 -> rsa_gfisr_spectral (rn + fpe + its
residual -> bf16 split planes) -> fdc 1x1 + GELU (three bf16 products in every policy, f32 map) -> irfft2 + post_norm, in place on the planes.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from . import lib as L
from . import lib_gfisr as LG
from . import ops
from .tensors import PF_BF16, Planes

EPS = 1e-6


class DftWorkspace(NamedTuple):
    scratch: torch.Tensor
    tabs: dict


def dft_workspace(plan, family: str, n: int, channels: int, H: int, W: int) -> DftWorkspace:
    """The scratch buffer and the tables of the H x W transforms of ``channels`` channels, kept by ``plan``."""
    nbytes = int(L.load().rsa_gfisr_dft_scratch_bytes(n, channels, H, W))
    if nbytes <= 0:
        raise RuntimeError(f'{family}: a {H}x{W} map is too large for the dense DFT (rsa_gfisr_dft)')
    ws = DftWorkspace(torch.empty(nbytes // 4, dtype=torch.float32, device=plan.device), LG.dft_tables(H, W, plan.device))
    plan.keep += [ws.scratch, *ws.tabs.values()]
    return ws


def emit_dft(plan, ws: DftWorkspace, inverse: bool, n: int, channels: int, H: int, W: int, spec, planes: Planes, plane0: int, post=None,
             eps: float = EPS) -> None:  # fmt: skip
    """rfft2 of ``planes`` (from ``plane0``) into ``spec``, or irfft2 of ``spec`` back into them; ``post``: the (scale, offset) of an RMSNorm
    the inverse transform applies to its result."""
    dp = LG.GfisrDftParams()
    dp.batch, dp.H, dp.W, dp.C, dp.inverse, dp.fmt, dp.eps = n, H, W, channels, int(inverse), planes.fmt, eps
    dp.tab_row = ws.tabs['row_inv' if inverse else 'row_fwd'].data_ptr()
    dp.tab_col = ws.tabs['col_inv' if inverse else 'col_fwd'].data_ptr()
    dp.spec, dp.scratch = spec.data_ptr(), ws.scratch.data_ptr()
    if post is not None:
        dp.norm_scale, dp.norm_offset = post[0].data_ptr(), post[1].data_ptr()
    planes.bind(dp, 'plane', plane0)
    Wf = W // 2 + 1
    flop = 2 * (H * W * 2 * Wf + 4 * H * H * Wf) * channels * n  # the row pass and the complex column pass
    unit = 2 * (2 if planes.lo is not None else 1)
    nbytes = n * channels * (H * W * unit + 2 * H * Wf * 4)
    label = f'{"inverse" if inverse else "forward"}{"" if post is None else " + post_norm"}, {H}x{W}, {channels} channels'
    plan.launch('rsa_gfisr_dft', dp, kernels=2, meta=dict(kernel='rsa_gfisr_dft', flop=flop, bytes=nbytes, label=label))


def _padded(t: torch.Tensor, rows: int, device) -> torch.Tensor:
    out = torch.zeros((rows, *t.shape[1:]), dtype=torch.float32, device=device)
    out[: t.shape[0]] = t
    return out.contiguous()


def pack_fourier_unit(sd: dict, fu: str, cf: int, rn, post, device) -> dict:
    """The FourierUnit under the key prefix ``fu`` over ``cf`` channels.  ``rn`` (2 cf spectral channels) and ``post`` (cf channels): the two
    RMSNorms as (scale, offset, eps) in the kernels' form, padded to whole planes here."""
    sp, fp = 8 * ((2 * cf + 7) // 8), 8 * ((cf + 7) // 8)
    blk = {'rn': (_padded(rn[0], sp, device), _padded(rn[1], sp, device), rn[2]), 'post': (_padded(post[0], fp, device), _padded(post[1], fp, device), post[2])}
    blk['fpe'] = (_padded(sd[f'{fu}.fpe.weight'].reshape(2 * cf, 9), sp, device), _padded(sd[f'{fu}.fpe.bias'], sp, device))
    # fdc's output row 2k is the real part of channel k and 2k + 1 its imaginary part: stored as [real of all | imag of all]
    rows = torch.cat([torch.arange(0, 2 * cf, 2), torch.arange(1, 2 * cf, 2)]).to(device)
    blk['fdc'] = ops.ConvWeights.from_oihw(sd[f'{fu}.fdc.weight'][rows], sd[f'{fu}.fdc.bias'][rows], 3, fmt=PF_BF16, device=device)
    return blk


def emit_fourier_unit(plan, blk: dict, ws: DftWorkspace, n: int, H: int, W: int, cf: int, planes: Planes, plane0: int, spec, sp_planes: Planes) -> None:
    """The FourierUnit on the ``cf`` channels of ``planes`` from ``plane0``, in place: ``spec`` is the f32 spectral map (2 cf channels, H x Wf),
    ``sp_planes`` the bf16 split planes fdc reads."""
    Wf = W // 2 + 1
    emit_dft(plan, ws, False, n, cf, H, W, spec, planes, plane0)
    scale, offset, eps = blk['rn']
    sp = LG.GfisrSpectralParams()
    sp.batch, sp.H, sp.W, sp.C, sp.eps = n, H, Wf, 2 * cf, eps
    sp.x, sp.scale, sp.offset = spec.data_ptr(), scale.data_ptr(), offset.data_ptr()
    sp.weight, sp.bias = blk['fpe'][0].data_ptr(), blk['fpe'][1].data_ptr()
    sp_planes.bind(sp, 'out')
    # byte model: the f32 map read once (the halo re-reads stay on chip), hi and lo planes written once
    plan.launch('rsa_gfisr_spectral', sp, meta=dict(kernel='rsa_gfisr_spectral', flop=0, bytes=n * H * Wf * (2 * cf * 4 + sp_planes.planes * 32)))
    plan.conv(ops.conv_params(blk['fdc'], sp_planes, H, Wf, act=L.ACT_GELU, out_f32=spec))
    emit_dft(plan, ws, True, n, cf, H, W, spec, planes, plane0, post=blk['post'][:2], eps=blk['post'][2])
