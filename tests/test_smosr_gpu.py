"""End-to-end GPU parity of SMoSR against the reference's vectors (tools/gen_golden_smosr.py).

Tolerance: max-abs <= 2e-4 * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3'; every fixture has |y|max >= 0.5
(tests/test_smosr_oracle.py), so that is a relative error of at most 4e-4.  The one-product 'fp16' mode is a benchmark mode, checked at
MoESR's looser bar.  Then the plan's shape, the byte model of the gate launch, and tiling.
"""

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd import tiling
from resselt_amd.archs.smosr.arch import SMoSR
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

MODEL_REL = 2e-4  # whole models: max-abs <= MODEL_REL * max(1, |y|max) (test_newer_archs_sweep_gpu.py prints its errors against it)

NAMES = golden_names('smosr_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _sd(meta):
    return synth.smosr_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures():
    assert len(NAMES) == 14


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert isinstance(m, SMoSR) and m.resolved_precision() == 'bf16x3'
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f})')
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
    print(f'MEASURE {name} fp16: max-abs {err:.3e}')
    assert err <= 3e-2 * max(1.0, arr['y'].abs().max().item())


class _Ops(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen.append(str(func))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize('name,stages', [('smosr_x2_psd_d48_rep0_9x11', 0), ('smosr_x4_pa_d48_rep1_m32_8x9', 2), ('smosr_x3_pa_d32_rep0_m24_n1_7x8', 1)])
def test_plan_shape(device, name, stages):
    """3 + n_mb launches of rsa_smosr_gate, one rsa_smosr_pa per pa_up stage, and no torch arithmetic on the forward path: what torch
    itself executes during a forward on the cached plan is the allocation of the output and the view that crops it."""
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    x = arr['x'].to(device)
    m(x)
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_smosr_gate') == 3 + meta['hyper']['n_mb'] and calls.count('rsa_smosr_pa') == stages
    with _Ops() as seen:
        m(x)
    torch.cuda.synchronize()
    views = ('aten.empty', 'aten.slice', 'aten.as_strided', 'aten.view', 'aten.alias', 'aten.detach', 'aten.select')
    assert all(op.startswith(views) for op in seen.seen), seen.seen


def test_gate_byte_model(device):
    """The first gate launch at 13 x 15 (9 x 11 padded by 2), dim 48, three products: a (2C) + s_in + s_out as f32, hi + lo planes."""
    meta, arr = load_golden('smosr_x2_psd_d48_rep0_9x11')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    priced = [meta_ for meta_, _ in m.last_plan().kernel_calls if meta_['kernel'] == 'rsa_smosr_gate']
    assert priced[0]['bytes'] == 13 * 15 * 48 * (8 + 4 + 4 + 2 + 2)
    # the last block of blocks_2 adds the trunk read; end_block.0 writes no stream
    assert priced[4]['bytes'] == 13 * 15 * 48 * (8 + 4 + 4 + 4 + 2 + 2) and priced[5]['bytes'] == 13 * 15 * 48 * (8 + 4 + 2 + 2)


def test_tiled_upscale_equals_untiled(device):
    sd = synth.smosr_state_dict(seed=31, head_gain=4.0)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    x = synth.synth_input((1, 3, 40, 40), 31).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    full = tiling.upscale(m, img, dtype=torch.float32)
    tiled = tiling.upscale(m, img, tile=(16, 24), halo=32, dtype=torch.float32)
    assert tiled.shape == full.shape == (80, 80, 3) and tiled.dtype == torch.uint8
    ymax = full.float().max().item() / 255
    assert (tiled.float() - full.float()).abs().max().item() / 255 <= MODEL_REL * max(1.0, ymax)
    # float tensors, a halo just above the network's reach (2 of the pad, 3 per SMB, 1 for end_block.1, 1 for the head: 22)
    yf = m(x)
    yt = tiling.upscale_tiled(m, x, 2, tile=(16, 24), halo=24)
    torch.cuda.synchronize()
    err = (yt - yf).abs().max().item()
    print(f'MEASURE tiled against untiled: {err:.3e}')
    assert err <= MODEL_REL * max(1.0, yf.abs().max().item())
