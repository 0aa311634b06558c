"""End-to-end GPU parity of RGT against the reference's vectors (tools/gen_golden_rgt.py) and the CPU oracle (tests/rgt_oracle.py).

Tolerance: max-abs <= 3e-4 * max(1, max|y|) in 'auto' (= 'bf16x3') and 'bf16x3'; the one-product 'bf16' mode at a looser bar; fp16
tensor I/O within 2e-3.
"""

import pytest
import torch

import resselt_amd
import rgt_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('rgt_')


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _tol(ref, rel=3e-4):
    return rel * max(1.0, ref.abs().max().item())


def _kw(meta):
    return {k: tuple(v) if isinstance(v, list) else v for k, v in meta['synth'].items()}


def _case(name):
    meta, arr = load_golden(name)
    kw = _kw(meta)
    sd = synth.rgt_state_dict(seed=meta['seed'], **kw)
    x = arr['x'] if 'x' in arr else arr['x_u8'].float() / 255
    y = arr['y'] if 'y' in arr else arr['y_crop']
    return sd, kw, x, y, 'y_crop' in arr


def _run(m, x, device, crop):
    y = m(x.to(device))
    torch.cuda.synchronize()
    return y[:, :, :32, :32].cpu() if crop else y.cpu()


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    sd, _, x, ref, crop = _case(name)
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
    sd, _, x, ref, crop = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = 'bf16'
    err = (_run(m, x, device, crop) - ref).abs().max().item()
    print(f'{name} bf16: max-abs {err:.3e}')
    assert err <= _tol(ref, 3e-2)


@pytest.mark.parametrize('name', [n for n in NAMES if 't3' not in n])
def test_fp16_io(device, name):
    sd, _, x, ref, _ = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    y = m(x.to(device).half())
    torch.cuda.synchronize()
    assert y.dtype == torch.float16
    err = (y.float().cpu() - ref).abs().max().item()
    assert err <= 2e-3 * max(1.0, ref.abs().max().item()), f'{name}: {err:.3e}'


@pytest.mark.parametrize('shape,kw', [
    ((1, 3, 512, 512), dict(embed_dim=36, depth=(2,), num_heads=(6,), split_size=(8, 32), upscale=2)),  # 1,024 pooled keys, t = 2
    ((1, 3, 256, 1024), dict(embed_dim=32, depth=(2,), num_heads=(2,), split_size=(4, 8), upscale=2)),  # t = 3: 4 x 16 keys
])  # fmt: skip
def test_matches_oracle_without_fixture(device, shape, kw):
    sd = synth.rgt_state_dict(seed=411, **kw)
    x = synth.synth_input(shape, 411)
    with torch.no_grad():
        ref = O.rgt_forward(sd, x, kw['split_size'], kw['num_heads'], 0.5)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    y = _run(m, x, device, False)
    err = (y - ref).abs().max().item()
    print(f'{shape}: max-abs {err:.3e}')
    assert err <= _tol(ref)


@pytest.mark.parametrize('hw,exc', [((15, 40), ValueError), ((40, 12), ValueError), ((16, 1100), RuntimeError)])
def test_sizes_the_reference_rejects_raise(device, hw, exc):
    sd = synth.rgt_state_dict(seed=412, embed_dim=32, depth=(2,), num_heads=(2,), split_size=(2, 4))
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    with pytest.raises(exc):
        m(torch.rand((1, 3) + hw, device=device))
