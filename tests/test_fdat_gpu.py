"""End-to-end GPU parity of FDAT against the reference's vectors (tools/gen_golden_fdat.py).

Tolerance: max-abs <= 3e-4 * max(1, max|y|) in 'auto' (= 'bf16x3') and 'bf16x3'; the one-product 'bf16' mode within 3e-2 * max(1, max|y|);
fp16 tensor I/O within 2e-3.  The unfused interaction path (interaction, residual add and norm2 as separate launches) agrees with the fused
one within 1e-5.  Larger inputs than the fixtures, embed_dim 180 included (the x4 transpose+conv head's first deconvolution then runs as two
cout slices), are checked against the CPU oracle (tests/fdat_oracle.py).
"""

import pytest
import torch

import resselt_amd
import fdat_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('fdat_')


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
    sd = synth.fdat_state_dict(seed=meta['seed'], **meta['synth'])
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
    assert torch.equal(_run(m, x, device, crop), y)  # the cached plan


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


@pytest.mark.parametrize('name', [n for n in NAMES if 'lda' in n or 'default' in n or 'b2' in n][:4])
def test_fused_and_unfused_interaction_agree(device, name):
    sd, x, ref, crop = _case(name)
    fused = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    unfused = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    unfused.fused_interact = False
    assert fused.fused_interact
    a, b = _run(fused, x, device, crop), _run(unfused, x, device, crop)
    assert (a - b).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    assert (b - ref).abs().max().item() <= _tol(ref)


def test_upscale_uint8(device):
    name = [n for n in NAMES if 'tconv_e48_w4_13x10' in n][0]
    sd, x, _, _ = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).to(device)
    out = resselt_amd.upscale(m, img)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2 * x.shape[2], 2 * x.shape[3], 3)
    y = m((img.permute(2, 0, 1)[None].float() / 255).to(device))
    want = (y.clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert (out.float() - want).abs().max().item() <= 1


@pytest.mark.parametrize('kw,shape', [
    (dict(embed_dim=180, num_heads=6, num_groups=1, depth_per_group=1, window_size=8, mid_dim=64, scale=4), (1, 3, 37, 30)),  # cout 180: two slices
    (dict(embed_dim=180, num_heads=6, num_groups=1, depth_per_group=1, window_size=8, mid_dim=64, scale=4, upsampler_type='lda'), (2, 3, 20, 17)),
    (dict(embed_dim=120, num_heads=4, num_groups=2, depth_per_group=1, window_size=16, mid_dim=64, scale=3, upsampler_type='pa_up'), (1, 3, 41, 35)),
    (dict(embed_dim=64, num_heads=4, num_groups=1, depth_per_group=2, window_size=8, mid_dim=32, scale=2, upsampler_type='transpose+conv',
          unshuffle_mod=True), (1, 3, 66, 51)),
])  # fmt: skip
def test_matches_oracle_without_fixture(device, kw, shape):
    sd = synth.fdat_state_dict(seed=531, **kw)
    x = synth.synth_input(shape, 531)
    with torch.no_grad():
        ref = O.fdat_forward(sd, x)
    for fused in (True, False):
        m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
        m.fused_interact = fused
        y = _run(m, x, device, None)
        assert y.shape == ref.shape
        err = (y - ref).abs().max().item()
        print(f'{kw} {shape} fused={fused}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
        assert err <= _tol(ref), err
