"""End-to-end GPU parity of EIMN against the reference's vectors (tools/gen_golden_eimn.py, eval mode) and, on larger inputs, the CPU oracle.

Tolerances (max-abs on the output image, |y|max 3.5 .. 6.4 on the fixtures; the ceiling of the three-product mode is the project's 1e-3).
Each is twice the largest deviation seen on the first GPU run over the six fixtures, rounded up to one significant digit -- twice, because
the fixtures are few and small:
    bf16x3 (= auto), fp32 I/O            measured 4.45e-5  -> 1e-4   (larger inputs against the oracle: 4.67e-5, the largest of both)
    bf16  (one product)                  measured 2.09e-2  -> 5e-2
    fp16  (one product)                  measured 2.68e-3  -> 6e-3
    bf16x3 with fp16 tensors             measured 5.30e-3  -> 2e-2   (the 16-stage fixture; 2.1e-3 .. 3.4e-3 on the 2- and 3-stage ones)
The fp16-tensor figure is the checkpoint's, not the kernels': the fp32 oracle on the CPU with the same checkpoint and input rounded to fp16
deviates from the reference's vector of the 16-stage fixture by 5.31e-3 (1.8e-3 .. 2.6e-3 on the others).
uint8 ``upscale()``: within one code of the oracle's quantised output.
"""

import pytest
import torch

import eimn_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('eimn_')
CEILING_BF16X3 = 1e-3
TOL_BF16X3, TOL_BF16, TOL_FP16, TOL_IO16 = 1e-4, 5e-2, 6e-3, 2e-2


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _case(name):
    meta, arr = load_golden(name)
    return synth.eimn_state_dict(seed=meta['seed'], **meta['synth']), arr['x'], arr['y'], meta.get('crop')


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
    if m.resolved_precision() == 'bf16x3':
        assert err <= CEILING_BF16X3
    assert torch.equal(_run(m, x, device, crop), y)  # the cached plan, bit for bit


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


@pytest.mark.parametrize('name', NAMES)
def test_uint8_upscale(device, name):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8)
    out = resselt_amd.upscale(m, img.to(device))
    assert out.dtype == torch.uint8
    with torch.no_grad():
        want = (O.eimn_forward(sd, (img.float() / 255).permute(2, 0, 1)[None]).clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert tuple(out.shape) == tuple(want.shape)
    diff = (out.cpu().int() - want.int()).abs().max().item()
    assert diff <= 1, diff


@pytest.mark.parametrize('kw,shape', [
    (dict(embed_dims=64, scale=2, num_stages=2), (1, 3, 61, 94)),
    (dict(embed_dims=48, scale=4, num_stages=2), (2, 3, 40, 72)),
])  # fmt: skip
def test_larger_inputs_against_the_oracle(device, kw, shape):
    sd = synth.eimn_state_dict(seed=41, **kw)
    x = synth.synth_input(shape, 41)
    with torch.no_grad():
        ref = O.eimn_forward(sd, x)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    y = _run(m, x, device, None)
    err = (y - ref).abs().max().item()
    print(f'MEASURE larger {kw} {shape}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert y.shape == ref.shape and err <= TOL_BF16X3 and err <= CEILING_BF16X3


def test_input_is_not_modified(device):
    sd, x, _, _ = _case(NAMES[0])
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xd = x.to(device)
    keep = xd.clone()
    m(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
