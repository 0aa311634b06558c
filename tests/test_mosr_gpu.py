"""End-to-end GPU parity of MoSR / MoSRv2 against the reference's vectors (tools/gen_golden_mosr.py) and the CPU oracle (tests/mosr_oracle.py).

Tolerance: max-abs <= 2e-4 * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3'.  The one-product 'fp16' mode is a benchmark
mode, checked at a looser bar.
"""

import pytest
import torch

import mosr_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('mosr_') + golden_names('mosrv2_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _tol(ref, rel=2e-4):
    return rel * max(1.0, ref.abs().max().item())


def _sd(meta):
    fn = synth.mosr_state_dict if meta['arch'] == 'mosr' else synth.mosrv2_state_dict
    return fn(seed=meta['seed'], **meta['synth'])


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
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


@pytest.mark.parametrize('scale', [1, 2])
def test_mosrv2_unshuffle_x1_and_x2_against_oracle(device, scale):
    """x1 with unshuffle_mod: no reference vector exists (the reference loader reads it as x4), so the oracle is the yardstick."""
    sd = synth.mosrv2_state_dict(scale=scale, n_block=2, dim=32, unshuffle_mod=True, seed=330 + scale)
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert m.parameters_info.upscale == scale and m.unshuffle == 4 // scale
    x = synth.synth_input((1, 3, 13, 18), 330 + scale)
    ref = O.mosrv2_forward(sd, x, 'pixelshuffledirect', scale)
    y = m.to(device)(x.to(device)).cpu()
    assert y.shape == ref.shape == (1, 3, 13 * scale, 18 * scale)
    err = (y - ref).abs().max().item()
    assert err <= _tol(ref), err


def test_load_from_file_pth_and_safetensors(device, tmp_path):
    pytest.importorskip('safetensors')
    from safetensors.torch import save_file

    for i, sd in enumerate((synth.mosr_state_dict(upscale=2, n_block=1, dim=32, seed=340), synth.mosrv2_state_dict(scale=2, n_block=1, dim=32, seed=341))):
        x = synth.synth_input((1, 3, 12, 12), 340 + i)
        outs = []
        for ext in ('pth', 'safetensors'):
            p = tmp_path / f'm{i}.{ext}'
            (torch.save(sd, p) if ext == 'pth' else save_file({k: v.contiguous() for k, v in sd.items()}, str(p)))
            m = resselt_amd.load_from_file(str(p)).to(device)
            assert m.parameters_info.upscale == 2
            outs.append(m(x.to(device)).cpu())
        assert outs[0].shape == (1, 3, 24, 24) and torch.equal(outs[0], outs[1])
