"""End-to-end GPU parity of GateR against the reference's vectors (tools/gen_golden_gater.py) and, on larger inputs, the CPU oracle.

Tolerances (max-abs; the outputs have |y|max 1.18 .. 1.52, the ceiling of the three-product mode is BASELINE's 1e-3 relative).  Each is
twice the largest deviation seen on the first GPU run over the seven fixtures, rounded up to one significant digit -- twice, because the
fixtures are few and small:
    bf16x3 (= auto), fp32 I/O            measured 1.38e-5  -> 3e-5   (larger inputs against the oracle: 1.39e-5)
    bf16  (one product)                  measured 7.72e-3  -> 2e-2
    fp16  (one product)                  measured 9.07e-4  -> 2e-3
    bf16x3 with fp16 tensors             measured 1.11e-3  -> 3e-3
The bf16x3 bound over the smallest |y|max is 3e-5 / 1.18 = 2.5e-5, far under the ceiling.
uint8 ``upscale()``: within one code of the oracle's quantised output.
"""

import pytest
import torch

import gater_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('gater_')
TOL_BF16X3, TOL_BF16, TOL_FP16, TOL_IO16 = 3e-5, 2e-2, 2e-3, 3e-3


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _case(name):
    meta, arr = load_golden(name)
    return synth.gater_state_dict(seed=meta['seed'], **meta['synth']), arr['x'], arr['y'], meta.get('crop')


def _run(m, x, device, crop):
    y = m(x.to(device))
    torch.cuda.synchronize()
    return (y[:, :, : crop[1], : crop[3]] if crop else y).float().cpu()


@pytest.mark.parametrize('precision,tol', [('auto', TOL_BF16X3), ('bf16x3', TOL_BF16X3), ('bf16', TOL_BF16), ('fp16', TOL_FP16)])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision, tol):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    y = _run(m, x, device, crop)
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= tol, f'{name} {precision}: max-abs {err:.3e}'
    assert torch.equal(_run(m, x, device, crop), y)  # the cached plan, bit for bit
    if precision in ('auto', 'bf16x3'):
        assert tol / ref.abs().max().item() < 1e-3  # BASELINE's ceiling for three-product mode


@pytest.mark.parametrize('name', NAMES)
def test_fp16_tensors(device, name):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device).half()
    y = m(x.half().to(device))
    assert y.dtype == torch.float16
    y = (y[:, :, : crop[1], : crop[3]] if crop else y).float().cpu()
    err = (y - ref).abs().max().item()
    print(f'MEASURE {name} io16: max-abs {err:.3e}')
    assert err <= TOL_IO16


@pytest.mark.parametrize('name', [n for n in NAMES if 'gray' not in n and '_n2_' not in n])
def test_uint8_upscale(device, name):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8)
    out = resselt_amd.upscale(m, img.to(device))
    assert out.dtype == torch.uint8
    with torch.no_grad():
        want = (O.gater_forward(sd, (img.float() / 255).permute(2, 0, 1)[None]).clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert tuple(out.shape) == tuple(want.shape)
    diff = (out.cpu().int() - want.int()).abs().max().item()
    assert diff <= 1, diff


@pytest.mark.parametrize('kw,shape', [
    (dict(dim=48, num_blocks=(1,) * 7, latent_att=True), (1, 3, 100, 72)),
    (dict(dim=48, num_blocks=(1,) * 7, latent_att=False), (2, 3, 61, 94)),
])  # fmt: skip
def test_larger_inputs_against_the_oracle(device, kw, shape):
    sd = synth.gater_state_dict(seed=31, **kw)
    x = synth.synth_input(shape, 31)
    with torch.no_grad():
        ref = O.gater_forward(sd, x)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    y = _run(m, x, device, None)
    err = (y - ref).abs().max().item()
    print(f'MEASURE larger {kw} {shape}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert y.shape == ref.shape and err <= TOL_BF16X3


def test_too_small_input_raises(device):
    sd, *_ = _case(NAMES[0])
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    with pytest.raises(RuntimeError, match='too small'):
        m(torch.zeros((1, 3, 4, 16), device=device))


def test_input_is_not_modified(device):
    sd, x, _, _ = _case('gater_d24_att_b2121212_9x9')
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xd = x.to(device)
    keep = xd.clone()
    m(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
