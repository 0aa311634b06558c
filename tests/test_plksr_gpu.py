"""End-to-end GPU parity of PLKSR / RealPLKSR against the reference's vectors (tools/gen_golden_plksr.py).

Tolerance: max-abs <= 2e-4 * max(1, max|y|), the bar of test_span_gpu.py, in 'auto' (= 'bf16x3' for this family) and 'bf16x3'.  The
one-product 'fp16' mode is a benchmark mode: checked at a looser bar so that its kernels (rsa_plk_conv and the streaming kernels on fp16
planes) run end to end.
"""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('plksr_') + golden_names('realplksr_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _tol(ref, rel=2e-4):
    return rel * max(1.0, ref.abs().max().item())


def _model(meta, device):
    fn = synth.plksr_state_dict if meta['arch'] == 'plksr' else synth.realplksr_state_dict
    return resselt_amd.load_from_state_dict(dict(fn(seed=meta['seed'], **meta['synth']))).to(device)


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
    y2 = m(arr['x'].to(device))  # second call: the cached plan (and, where enabled, its graph replay)
    assert torch.equal(y2, y)


@pytest.mark.parametrize('name', NAMES)
def test_fp16_mode_runs(device, name):
    meta, arr = load_golden(name)
    m = _model(meta, device)
    m.precision = 'fp16'
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    err = (y.float().cpu() - arr['y']).abs().max().item()
    print(f'{name} fp16: max-abs {err:.3e}')
    assert err <= _tol(arr['y'], 2e-2)


def test_deep_realplksr_auto_equals_bf16x3(device):
    sd = synth.realplksr_state_dict(dim=64, n_blocks=28, upscale=4, seed=7)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    x = synth.synth_input((1, 3, 256, 256), 7).to(device)
    y_auto = m(x)
    m.precision = 'bf16x3'
    y_ref = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y_ref).all()
    assert (y_auto - y_ref).abs().max().item() <= _tol(y_ref)


def test_realplksr_batch_matches_single_images(device):
    """GroupNorm statistics are per image: a batch of two equals the two images run alone."""
    meta, arr = load_golden('realplksr_x4_dys_d32_b1_b2_12x16')
    m = _model(meta, device)
    x = arr['x'].to(device)
    yb = m(x)
    y0, y1 = m(x[:1].contiguous()), m(x[1:].contiguous())
    torch.cuda.synchronize()
    assert (yb - torch.cat([y0, y1])).abs().max().item() <= 1e-6 * max(1.0, yb.abs().max().item())
