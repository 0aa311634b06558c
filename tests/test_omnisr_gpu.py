"""End-to-end GPU parity of OmniSR against the reference's vectors (tools/gen_golden_omnisr.py).

Tolerance: max-abs <= 3e-4 * max(1, max|y|) in 'auto' (= 'bf16x3') and 'bf16x3'; the one-product 'bf16' mode within 3e-2 * max(1, max|y|);
fp16 tensor I/O within 2e-3.  Larger inputs than the fixtures (several 64-token chunks per grid residue class, grid strides up to 12,
ESA maps of several pixels) are checked against the CPU oracle (tests/omnisr_oracle.py) with sharpened channel-attention temperatures.  An input whose padded side is below 15 raises RuntimeError (as the reference's ESA max-pool does) before any
launch.
"""

import pytest
import torch

import resselt_amd
import omnisr_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('omnisr_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _tol(ref, rel=3e-4):
    return rel * max(1.0, ref.abs().max().item())


def _case(name):
    meta, arr = load_golden(name)
    sd = synth.omnisr_state_dict(seed=meta['seed'], **meta['synth'])
    return sd, arr['x'], arr['y'], meta.get('crop')


def _run(m, x, device, crop):
    y = m(x.to(device))
    torch.cuda.synchronize()
    return (y[:, :, : crop[1], : crop[3]] if crop else y).float().cpu()


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    assert m.resolved_precision() == 'bf16x3'
    y = _run(m, x, device, crop)
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    print(f'{name} {precision}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= _tol(ref), f'{name} {precision}: max-abs {err:.3e}'
    assert torch.equal(_run(m, x, device, crop), y)  # the cached plan, bit for bit


@pytest.mark.parametrize('name', NAMES)
def test_bf16_mode(device, name):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = 'bf16'
    err = (_run(m, x, device, crop) - ref).abs().max().item()
    print(f'{name} bf16: max-abs {err:.3e}')
    assert err <= _tol(ref, 3e-2)


@pytest.mark.parametrize('name', NAMES)
def test_fp16_io(device, name):
    sd, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    y = m(x.to(device).half())
    torch.cuda.synchronize()
    assert y.dtype == torch.float16
    if crop:
        y = y[:, :, : crop[1], : crop[3]]
    err = (y.float().cpu() - ref).abs().max().item()
    assert err <= 2e-3 * max(1.0, ref.abs().max().item()), f'{name}: {err:.3e}'


def test_upscale_uint8(device):
    name = [n for n in NAMES if 'x2_c32_w4_25x17' in n][0]
    sd, x, _, _ = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).to(device)
    out = resselt_amd.upscale(m, img)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2 * x.shape[2], 2 * x.shape[3], 3)
    y = m((img.permute(2, 0, 1)[None].float() / 255).to(device))
    want = (y.clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert (out.float() - want).abs().max().item() <= 1


@pytest.mark.parametrize('shape', [(1, 3, 8, 20), (1, 3, 20, 7)])
def test_too_small_input_raises_before_any_launch(device, shape):
    sd = synth.omnisr_state_dict(num_feat=32, window_size=8, up_scale=2, seed=3)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='ESA'):
        m(torch.rand(shape, device=device))
    torch.cuda.synchronize()
    assert L.load().rsa_check_status() == 0


@pytest.mark.parametrize('kw,shape', [
    (dict(num_feat=64, res_num=2, block_num=1, pe=True, window_size=8, up_scale=4), (1, 3, 64, 80)),
    (dict(num_feat=48, res_num=1, block_num=2, pe=True, window_size=8, up_scale=2), (1, 3, 100, 72)),
    (dict(num_feat=64, res_num=1, block_num=1, pe=False, window_size=8, up_scale=3), (2, 3, 100, 72)),
    (dict(num_feat=32, res_num=1, block_num=1, pe=True, window_size=4, up_scale=2, bias=False), (1, 3, 61, 94)),
])  # fmt: skip
@pytest.mark.parametrize('precision', ['bf16x3', 'bf16'])
def test_matches_oracle_without_fixture(device, kw, shape, precision):
    sd = synth.omnisr_state_dict(seed=641, **kw)
    for k in sd:
        if k.endswith('temperature'):
            sd[k] = sd[k] * 8.0  # sharp channel-attention softmaxes, not near-uniform ones
    x = synth.synth_input(shape, 641)
    with torch.no_grad():
        ref = O.omnisr_forward(sd, x)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    y = _run(m, x, device, None)
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    print(f'{kw} {shape} {precision}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= _tol(ref, 3e-4 if precision == 'bf16x3' else 3e-2), err
