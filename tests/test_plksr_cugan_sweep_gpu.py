"""PLKSR, RealPLKSR and Real-CUGAN on the GPU against their CPU oracles (oracle/plksr.py, oracle/cugan.py) at shapes the golden fixtures do
not reach: every residue of the CUGAN input height and width that reaches its grids (from the minimum legal size up), a medium frame per
variant and both benchmarked frames; PLKSR images smaller than, around and far larger than the large kernel, every mixer / large-kernel type, both heads
at x1..x4.

Tolerance: max-abs <= 2e-4 * max(1, max|y|), the bar of test_plksr_gpu.py and test_cugan_gpu.py, in 'auto' (= 'bf16x3' for both families)
and 'bf16x3'; fp16 / bf16 tensors in and out at the 1e-2 bar of test_cugan_gpu.test_half_and_bfloat16_io.  The oracle runs in float64 for
small frames and in fp32 for the large ones.  Every case calls the model twice and asserts that the cached plan gives the same bits.
"""

import pytest
import torch

import resselt_amd
from oracle.cugan import cugan_forward
from oracle.plksr import plksr_forward
from resselt_amd.archs.cugan.arch import cugan_layers
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _oracle(sd, x, fwd, f64):
    dt = torch.float64 if f64 else torch.float32
    with torch.no_grad():
        return fwd({k: v.to(dt) for k, v in sd.items()}, x.to(dt)).to(torch.float64)


def _check(m, sd, x, fwd, device, *, precision='auto', f64=True, rel=2e-4, what=''):
    """Run ``x`` (any dtype) twice on ``m``; compare the first output with the oracle on the same values, the second with the first."""
    ref = _oracle(sd, x.float(), fwd, f64)
    m.precision = precision
    xd = x.to(device)
    y = m(xd)
    torch.cuda.synchronize()
    assert y.shape == ref.shape and y.dtype == x.dtype, what
    err = (y.cpu().to(torch.float64) - ref).abs().max().item()
    tol = rel * max(1.0, ref.abs().max().item())
    print(f'{what} {tuple(x.shape)} {str(x.dtype)[6:]} {precision}: max-abs {err:.3e} / tol {tol:.3e} = {err / tol:.3f}')
    assert err <= tol, f'{what} {tuple(x.shape)}: max-abs {err:.3e} > {tol:.3e}'
    assert torch.equal(m(xd), y), f'{what}: the cached plan gave different bits'


# ---------------------------------------------------------------------------------------------------------------- Real-CUGAN
def _legal(variant, w0, count):
    return [h for h in range(1, 200) if _accepts(variant, h, w0)][:count]


def _accepts(variant, h0, w0):
    try:
        cugan_layers(variant, 3, 3, h0, w0)
    except ValueError:
        return False
    return True


def _cugan(variant, pro, seed, device):
    sd = synth.cugan_state_dict(variant, pro=pro, seed=seed)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    assert m.resolved_precision() == 'bf16x3'
    return sd, m


def _two_images(shape, seed):
    x = synth.synth_input(shape, seed=seed)
    if shape[0] > 1:
        x[1] = x[1] * 0.5 + 0.25  # another image statistic: the SE means are per image
    return x


# w0 of another residue than most of the heights: odd for the multiple-of-2 variants, 2 mod 4 for 3x, 3 mod 4 for 2x_fast
SWEEP_W = {'2x': 27, '3x': 30, '4x': 25, '2x_fast': 47}


@pytest.mark.parametrize('axis', ['h', 'w'])
@pytest.mark.parametrize('variant', ['2x', '3x', '4x', '2x_fast'])
def test_cugan_consecutive_sizes(device, variant, axis):
    """Eight consecutive legal heights (widths) from the minimum -- every residue the pad multiple, the halvings and the crops see -- with
    the other side fixed at another residue; the first size in a batch of two, the precisions alternating."""
    sd, m = _cugan(variant, False, 41, device)
    other = SWEEP_W[variant]
    sides = _legal(variant, other, 8)
    assert len(sides) == 8 and not _accepts(variant, sides[0] - 1, other)
    for i, s in enumerate(sides):
        hw = (s, other) if axis == 'h' else (other, s)
        x = _two_images((2 if i == 0 else 1, 3, *hw), seed=s)
        _check(m, sd, x, cugan_forward, device, precision=('auto', 'bf16x3')[i % 2], what=f'cugan {variant}')


@pytest.mark.parametrize('variant', ['2x', '3x', '4x'])
def test_cugan_pro_sizes(device, variant):
    sd, m = _cugan(variant, True, 43, device)
    hs = _legal(variant, 33, 3)
    for i, (h0, w0) in enumerate([(hs[0], 33), (hs[1], 30), (hs[2], 41)]):
        x = _two_images((2 if i == 1 else 1, 3, h0, w0), seed=100 + h0)
        _check(m, sd, x, cugan_forward, device, precision=('auto', 'bf16x3')[i % 2], what=f'cugan {variant} pro')


@pytest.mark.parametrize('variant', ['2x', '3x', '4x', '2x_fast'])
def test_cugan_half_and_bfloat16_io(device, variant):
    sd, m = _cugan(variant, variant == '3x', 45, device)
    h0 = _legal(variant, 44, 3)[-1]
    for dt in (torch.float16, torch.bfloat16):
        x = synth.synth_input((1, 3, h0, 44), seed=7).to(dt)
        _check(m, sd, x, cugan_forward, device, rel=1e-2, what=f'cugan {variant}')


@pytest.mark.parametrize('variant, shape', [('2x', (1, 3, 200, 300)), ('3x', (1, 3, 203, 298)), ('4x', (2, 3, 201, 299)),
                                            ('2x_fast', (1, 3, 199, 300)), ('4x', (1, 3, 540, 960)), ('2x', (1, 3, 1080, 1920))])  # fmt: skip
def test_cugan_large_frames(device, variant, shape):
    """Many workgroups per layer and ragged last tiles; the two benchmarked frames, 4x at 540x960 and 2x at 1080x1920 (their fp32 CPU
    oracles take seconds)."""
    sd, m = _cugan(variant, False, 47, device)
    _check(m, sd, _two_images(shape, seed=shape[2]), cugan_forward, device, f64=False, what=f'cugan {variant}')


# ---------------------------------------------------------------------------------------------------------------- PLKSR / RealPLKSR
SMALL = [(1, 1), (1, 40), (40, 1), (5, 7), (16, 17), (33, 31)]


@pytest.mark.parametrize('ccm, lk, k', [('DCCM', 'PLK', 17), ('CCM', 'PLK', 31), ('ICCM', 'PLK', 9), ('DCCM', 'SparsePLK', 17),
                                        ('CCM', 'RectSparsePLK', 17), ('ICCM', 'RectSparsePLK', 9)])  # fmt: skip
def test_plksr_small_images(device, ccm, lk, k):
    """Images below, around and just above the kernel, for every mixer and large-kernel type."""
    sd = synth.plksr_state_dict(dim=32, n_blocks=2, upscale=2, ccm_type=ccm, kernel_size=k, lk_type=lk, use_ea=ccm != 'ICCM', seed=k)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    for i, (h, w) in enumerate(SMALL):
        _check(m, sd, synth.synth_input((1, 3, h, w), seed=h * 100 + w), plksr_forward, device, precision=('auto', 'bf16x3')[i % 2],
               what=f'plksr {ccm} {lk} k{k}')  # fmt: skip


@pytest.mark.parametrize('upscale', [1, 2, 3, 4])
@pytest.mark.parametrize('dysample', [False, True])
def test_realplksr_heads(device, upscale, dysample):
    """Both heads at every scale, a batch of three with per-image GroupNorm statistics, small and ragged sizes."""
    sd = synth.realplksr_state_dict(dim=32, n_blocks=2, upscale=upscale, dysample=dysample, seed=upscale)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    for i, (h, w) in enumerate([(5, 7), (1, 40), (21, 18)]):
        x = synth.synth_input((3, 3, h, w), seed=i)
        x[1], x[2] = x[1] * 0.3 + 0.6, x[2] * 2.0 - 0.5
        _check(m, sd, x, plksr_forward, device, precision=('auto', 'bf16x3')[i % 2], what=f'realplksr x{upscale} dys={dysample}')


@pytest.mark.parametrize('k, pdim', [(9, 8), (17, 16), (31, 64)])
def test_realplksr_kernel_sizes_and_pdim(device, k, pdim):
    sd = synth.realplksr_state_dict(dim=64, n_blocks=1, upscale=2, kernel_size=k, split_ratio=pdim / 64, seed=k)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    assert m.pdim == pdim
    for i, (h, w) in enumerate([(5, 7), (16, 17), (40, 1)]):
        _check(m, sd, synth.synth_input((1, 3, h, w), seed=k + i), plksr_forward, device, precision=('auto', 'bf16x3')[i % 2],
               what=f'realplksr k{k} pdim{pdim}')  # fmt: skip


@pytest.mark.parametrize('arch, kw', [
    ('plksr', dict(ccm_type='DCCM', lk_type='SparsePLK', upscale=3)),
    ('plksr', dict(ccm_type='CCM', lk_type='RectSparsePLK', upscale=4)),
    ('realplksr', dict(upscale=2, dysample=True, kernel_size=31)),
    ('realplksr', dict(upscale=4)),
])  # fmt: skip
def test_plksr_many_tiles(device, arch, kw):
    """Several PLK_TW x PLK_TH tiles with ragged right and bottom edges."""
    make = synth.plksr_state_dict if arch == 'plksr' else synth.realplksr_state_dict
    sd = make(dim=32, n_blocks=2, seed=3, **kw)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    _check(m, sd, synth.synth_input((1, 3, 70, 150), seed=3), plksr_forward, device, f64=False, what=f'{arch} {kw}')
