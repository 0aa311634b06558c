"""End-to-end GPU parity of RCAN against the reference's vectors (tools/gen_golden_rcan.py) and, on larger inputs, the CPU oracle.

Tolerances (max-abs on the 0..1 output image; the ceiling of the three-product mode is BASELINE's 1e-3).  Each is twice the largest
deviation seen on the first GPU run over the nine fixtures, rounded up to one significant digit -- twice, because the fixtures are few
and small:
    bf16x3 (= auto), fp32 I/O            measured 4.86e-6  -> 1e-5   (larger inputs against the oracle: 3.70e-6)
    bf16  (one product)                  measured 2.55e-3  -> 6e-3
    fp16  (one product)                  measured 2.93e-4  -> 6e-4
    bf16x3 with fp16 tensors             measured 3.97e-4  -> 8e-4
    fused against composed, bf16x3       measured 2.00e-6  -> 4e-6   (the pooled sum's order is the only difference)
    fused against composed, fp16         measured 1.26e-4  -> 3e-4   (a last-bit change of a gate moves fp16-rounded activations by an ulp)
uint8 ``upscale()``: within one code of the reference's quantised output.
"""

import pytest
import torch

import rcan_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('rcan_')
TOL_BF16X3, TOL_BF16, TOL_FP16, TOL_IO16 = 1e-5, 6e-3, 6e-4, 8e-4
TOL_FUSED = {'bf16x3': 4e-6, 'fp16': 3e-4}


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _case(name):
    meta, arr = load_golden(name)
    return synth.rcan_state_dict(seed=meta['seed'], **meta['synth']), arr['x'], arr['y'], meta.get('crop')


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
    print(f'MEASURE {name} {precision} fused={m.rcan_fused_active}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= tol, f'{name} {precision}: max-abs {err:.3e}'
    assert torch.equal(_run(m, x, device, crop), y)  # the cached plan, bit for bit
    assert m.rcan_fused_active == (m.n_feats in (48, 64) and precision != 'bf16')


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


@pytest.mark.parametrize('name', [n for n in NAMES if 'gray' not in n])
def test_uint8_upscale(device, name):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8)
    out = resselt_amd.upscale(m, img.to(device))
    assert out.dtype == torch.uint8
    with torch.no_grad():
        want = (O.rcan_forward(sd, (img.float() / 255).permute(2, 0, 1)[None]).clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert tuple(out.shape) == tuple(want.shape)
    diff = (out.cpu().int() - want.int()).abs().max().item()
    assert diff <= 1, diff


@pytest.mark.parametrize('kw,shape', [
    (dict(scale=2, n_resgroups=2, n_resblocks=2), (1, 3, 100, 72)),
    (dict(scale=4, n_resgroups=1, n_resblocks=3, n_feats=48, reduction=8), (2, 3, 61, 94)),
    (dict(scale=2, n_resgroups=1, n_resblocks=2, unshuffle_mod=True), (1, 3, 61, 94)),
])  # fmt: skip
def test_larger_inputs_against_the_oracle(device, kw, shape):
    sd = synth.rcan_state_dict(seed=31, **kw)
    x = synth.synth_input(shape, 31)
    with torch.no_grad():
        ref = O.rcan_forward(sd, x)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    y = _run(m, x, device, None)
    assert m.rcan_fused_active
    err = (y - ref).abs().max().item()
    print(f'MEASURE larger {kw} {shape}: max-abs {err:.3e}')
    assert y.shape == ref.shape and err <= TOL_BF16X3


@pytest.mark.parametrize('precision', ['bf16x3', 'fp16'])
@pytest.mark.parametrize('name', NAMES)
def test_fused_against_composed(device, name, precision):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    fused = _run(m, x, device, crop)
    was_fused = m.rcan_fused_active
    m.rcan_fused = False
    m.invalidate()
    composed = _run(m, x, device, crop)
    assert not m.rcan_fused_active
    err = (fused - composed).abs().max().item()
    print(f'MEASURE {name} {precision} fused-vs-composed (fused={was_fused}): max-abs {err:.3e}')
    assert err <= TOL_FUSED[precision]
    if not was_fused:
        assert torch.equal(fused, composed)


def test_input_is_not_modified(device):
    sd, x, _, _ = _case(NAMES[0])
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xd = x.to(device)
    keep = xd.clone()
    m(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
