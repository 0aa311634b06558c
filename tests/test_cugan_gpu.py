"""End-to-end GPU parity of Real-CUGAN against the reference's vectors (tools/gen_golden_cugan.py).

Tolerance: max-abs <= 2e-4 * max(1, max|y|), the bar of test_plksr_gpu.py, in 'auto' (= 'bf16x3' for this family) and 'bf16x3'.  The
one-product 'fp16' mode is a benchmark mode, checked at 2e-2.
"""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('cugan_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _tol(ref, rel=2e-4):
    return rel * max(1.0, ref.abs().max().item())


def _model(meta, device):
    return resselt_amd.load_from_state_dict(dict(synth.cugan_state_dict(seed=meta['seed'], **meta['synth']))).to(device)


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = _model(meta, device)
    assert m.resolved_precision() == 'bf16x3'
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'{name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f})')
    assert err <= _tol(arr['y']), f'{name} {precision}: max-abs {err:.3e}'
    y2 = m(arr['x'].to(device))  # second call: the cached plan
    assert torch.equal(y2, y)
    n = m.launches_per_forward()
    se = sum(1 for k in m.state_dict() if k.endswith('seblock.conv1.weight'))
    assert n == m.last_plan().n_launches() and n > 3 * se


@pytest.mark.parametrize('name', NAMES)
def test_fp16_mode_runs(device, name):
    meta, arr = load_golden(name)
    m = _model(meta, device)
    m.precision = 'fp16'
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'{name} fp16: max-abs {err:.3e}')
    assert err <= _tol(arr['y'], 2e-2)


@pytest.mark.parametrize('variant', ['2x', '4x'])
def test_batch_equals_single_images(device, variant):
    m = resselt_amd.load_from_state_dict(dict(synth.cugan_state_dict(variant, seed=9))).to(device)
    x = synth.synth_input((2, 3, 22, 26), seed=9).to(device)
    x[1] = x[1] * 0.5 + 0.25  # a different image statistic: SE means are per image
    y = m(x)
    y0, y1 = m(x[:1].contiguous()), m(x[1:].contiguous())
    assert torch.equal(y[:1], y0) and torch.equal(y[1:], y1)


@pytest.mark.parametrize('name', ['cugan_x2_23x22', 'cugan_x4_pro_b2_20x24'])
def test_upscale_u8_round_trip(device, name):
    from resselt_amd.tiling import upscale

    meta, arr = load_golden(name)
    m = _model(meta, device)
    img = (arr['x'] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    y8 = upscale(m, img.to(device))
    torch.cuda.synchronize()
    # the same model on the f32 image that the bytes stand for
    yf = m((img.permute(0, 3, 1, 2).float() / 255).to(device))
    ref8 = (yf.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu()
    assert y8.dtype == torch.uint8 and y8.shape == ref8.shape
    assert (y8.cpu().int() - ref8.int()).abs().max().item() <= 1
    assert (y8.cpu() != ref8).float().mean().item() < 1e-3


def test_half_and_bfloat16_io(device):
    meta, arr = load_golden('cugan_x3_18x18')
    m = _model(meta, device)
    for dt in (torch.float16, torch.bfloat16):
        y = m(arr['x'].to(device).to(dt))
        assert y.dtype == dt
        assert (y.float().cpu() - arr['y']).abs().max().item() <= 1e-2 * max(1.0, arr['y'].abs().max().item())


def test_too_small_input_raises_before_launch(device):
    m = resselt_amd.load_from_state_dict(dict(synth.cugan_state_dict('2x_fast'))).to(device)
    with pytest.raises(ValueError):
        m(torch.rand(1, 3, 42, 46, device=device))
    assert m.launches_per_forward() is None
