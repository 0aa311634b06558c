"""End-to-end GPU parity of MoESR against the reference's vectors (tools/gen_golden_moesr.py).

Tolerance: max-abs <= 2e-4 * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3'.  The one-product 'fp16' mode is a benchmark
mode, checked at a looser bar.  moesr_x4_full_d64_g9b4_9x11 is the depth check: the default 9 x (4 + 3) = 63 gated blocks of accumulated
error on the f32 stream meet the same 2e-4 bar.
"""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs.moesr.arch import MoESR
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

MODEL_REL = 2e-4  # whole models: max-abs <= MODEL_REL * max(1, |y|max) (test_newer_archs_sweep_gpu.py prints its errors against it)

NAMES = golden_names('moesr_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _sd(meta):
    return synth.moesr_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures():
    assert len(NAMES) == 7


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert isinstance(m, MoESR) and m.resolved_precision() == 'bf16x3'
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'{name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f})')
    assert err <= MODEL_REL * max(1.0, arr['y'].abs().max().item()), f'{name} {precision}: max-abs {err:.3e}'
    y2 = m(arr['x'].to(device))  # second call: the cached plan
    assert torch.equal(y2, y)


@pytest.mark.parametrize('name', NAMES)
def test_fp16_mode_runs(device, name):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m.precision = 'fp16'
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape and torch.isfinite(y).all()
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'{name} fp16: max-abs {err:.3e}')
    assert err <= 3e-2 * max(1.0, arr['y'].abs().max().item())


def test_one_stream_launch_per_block_and_resolution_change(device):
    """The plan's shape: per group n_block + 3 block tails, one MSG entry and one MSG exit, and a single rsa_layernorm in the whole model."""
    meta, arr = load_golden('moesr_x2_psd_d32_g2b1_9x11')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_moesr_stream') == 2 * (1 + 3 + 2) and calls.count('rsa_gated_dwconv') == 2 * (1 + 3)
    priced = [meta_ for meta_, _ in m.last_plan().kernel_calls if meta_['kernel'] == 'rsa_moesr_stream']
    # the first block tail at 10 x 12 (9 x 11 padded), dim 32, three products: a + s_in + s_out as f32, plain hi + lo planes
    assert priced[0]['bytes'] == 10 * 12 * 32 * (4 * 3 + 2 * 2)
    # the MSG entry at 5 x 6: a + s_out, LayerNorm hi + lo planes
    assert priced[1]['bytes'] == 5 * 6 * 32 * (4 * 2 + 2 * 2)


def test_load_from_file_pth_and_safetensors(device, tmp_path):
    pytest.importorskip('safetensors')
    from safetensors.torch import save_file

    sd = synth.moesr_state_dict(scale=2, dim=32, n_blocks=1, n_block=1, seed=1140)
    x = synth.synth_input((1, 3, 11, 12), 1140)
    outs = []
    for ext in ('pth', 'safetensors'):
        p = tmp_path / f'm.{ext}'
        (torch.save(sd, p) if ext == 'pth' else save_file({k: v.contiguous() for k, v in sd.items()}, str(p)))
        m = resselt_amd.load_from_file(str(p)).to(device)
        assert m.parameters_info.upscale == 2 and m.parameters_info.name == 'MoESR'
        outs.append(m(x.to(device)).cpu())
    assert outs[0].shape == (1, 3, 22, 24) and torch.equal(outs[0], outs[1])
