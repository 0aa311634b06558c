"""End-to-end GPU parity of RHA against the reference's vectors (tools/gen_golden_rha.py: the reference's f32 CPU output in eval mode).

Tolerances (max-abs on the output image, |y|max 0.36 .. 0.88 on the fixtures).  Each is twice the largest deviation seen on the first GPU
run over the six fixtures (the batch-2 and second-size cases against the oracle included: 8.86e-6, the largest of all); under bf16x3 the error must in any case stay within the project's 1e-3 of max(1, |y|max) -- above that it is a
bug, not a tolerance:
    bf16x3 (= auto), fp32 I/O            measured 8.27e-6 (8.86e-6) -> 1.8e-5
    bf16  (one product)                  measured 4.94e-3           -> 9.9e-3
    fp16  (one product)                  measured 5.73e-4           -> 1.15e-3
    bf16x3 with fp16 tensors             measured 7.18e-4           -> 1.44e-3
    bf16x3 with bf16 tensors             measured 3.69e-3           -> 7.4e-3
"""

import pytest
import torch

import rha_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('rha_')
CEILING_BF16X3 = 1e-3
TOL_BF16X3, TOL_BF16, TOL_FP16, TOL_IO16, TOL_IOBF = 1.8e-5, 9.9e-3, 1.15e-3, 1.44e-3, 7.4e-3


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _sd(meta):
    kw = dict(meta['synth'])
    kw['down_list'] = tuple(kw['down_list'])
    return synth.rha_state_dict(seed=meta['seed'], **kw)


def _case(name):
    meta, arr = load_golden(name)
    return _sd(meta), arr['x'], arr['y'], meta.get('crop'), meta


def _crop(y, crop):
    return (y[:, :, : crop[1], : crop[3]] if crop else y).float().cpu()


def _run(m, x, device, crop):
    y = m(x.to(device))
    torch.cuda.synchronize()
    return _crop(y, crop)


@pytest.mark.parametrize('precision,tol', [('auto', TOL_BF16X3), ('bf16x3', TOL_BF16X3), ('bf16', TOL_BF16), ('fp16', TOL_FP16)])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision, tol):
    sd, x, ref, crop, meta = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    y = _run(m, x, device, crop)
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= tol, f'{name} {precision}: max-abs {err:.3e}'
    if m.resolved_precision() == 'bf16x3':
        assert err <= CEILING_BF16X3 * max(1.0, meta['y_absmax'])
    assert torch.equal(_run(m, x, device, crop), y)  # the cached plan, bit for bit


@pytest.mark.parametrize('dt,tol', [(torch.float16, TOL_IO16), (torch.bfloat16, TOL_IOBF)])
@pytest.mark.parametrize('name', NAMES)
def test_half_tensors(device, name, dt, tol):
    sd, x, ref, crop, _ = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device).to(dt)
    y = m(x.to(dt).to(device))
    assert y.dtype == dt
    err = (_crop(y, crop) - ref).abs().max().item()
    print(f'MEASURE {name} io {dt}: max-abs {err:.3e}')
    assert err <= tol


def test_batch_two_and_a_second_size_on_the_same_module(device):
    """Batch 2 of different images against the oracle, then another size through the same module (a second plan), then the first again."""
    sd, x, _, _, _ = _case('rha_x2_psd_d32_dn21_g2b2_13x18')
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    x2 = torch.cat((x, synth.synth_input(x.shape, 5)), 0)
    x3 = synth.synth_input((1, 3, 21, 40), 6)  # pads to 32 x 48: 2 x 3 windows of the pooled map at down 2, 1 x 1.5 -> 2 x 3 of 16 x 24
    with torch.no_grad():
        r2, r3 = O.rha_forward(sd, x2), O.rha_forward(sd, x3)
    y2 = _run(m, x2, device, None)
    y3 = _run(m, x3, device, None)
    e2, e3 = (y2 - r2).abs().max().item(), (y3 - r3).abs().max().item()
    print(f'MEASURE batch 2: {e2:.3e}; second size: {e3:.3e}')
    assert y2.shape == r2.shape and y3.shape == r3.shape
    assert e2 <= TOL_BF16X3 and e3 <= TOL_BF16X3
    assert torch.equal(_run(m, x2, device, None), y2)


def test_input_is_not_modified_and_small_inputs_are_refused(device):
    sd, x, _, _, _ = _case(NAMES[0])
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xd = x.to(device)
    keep = xd.clone()
    m(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
    with pytest.raises(RuntimeError, match='too small'):
        m(torch.zeros((1, x.shape[1], 3, 40), device=device))
