"""The CPU oracle of LAWFFT (tests/lawfft_oracle.py) against the reference's vectors (tools/gen_golden_lawfft.py), its FFT form of the
correlation against its direct-sum form, and the sizes of the probe fixture that the reference runs.

The oracle in float32 against every fixture: max-abs <= 4 * the fixture's own ``f64_dev`` (the deviation of the reference's f32 forward,
which the fixture stores, from its forward on a ``.double()`` copy), floored at 1e-6 * max(1, |y|max); the margin covers FFT-library
differences.  The FFT form against the direct sum in float64: 1e-12 relative to the largest correlation."""

import pytest
import torch
import torch.nn.functional as F

import lawfft_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = [n for n in golden_names('lawfft_') if n != 'lawfft_probe']


def bar_of(meta) -> float:
    return max(4.0 * meta['f64_dev'], 1e-6 * max(1.0, meta['y_absmax']))


def test_fixtures_cover_what_the_issue_lists():
    metas = [load_golden(n)[0] for n in NAMES]
    hy = [m['hyper'] for m in metas]
    shapes = [tuple(load_golden(n)[1]['x'].shape) for n in NAMES]
    assert len(NAMES) == 11
    default = [i for i, h in enumerate(hy) if (h['dim'], h['n_rblock'], h['n_mblock'], h['scale'], h['upsampler']) == (60, 4, 6, 4, 'pixelshuffledirect')]
    assert default and shapes[default[0]] == (1, 3, 9, 11)
    assert {h['upsampler'] for h in hy} == set(O.MODES) and {h['scale'] for h in hy} == {1, 2, 3, 4}
    assert any(s[0] == 2 for s in shapes) and {h['n_mblock'] for h in hy} >= {2, 3}
    widths = {(m['hyper']['dim'], m['synth'].get('local', 15)) for m in metas}
    assert (64, 16) in widths and (60, 15) in widths
    assert any(h['t_mid_factor'] != 1.0 for h in hy) and any(abs(h['mlp_factor'] - 2.66) > 0.05 for h in hy)
    assert (2, 3, 8, 16) in shapes and (1, 3, 9, 17) in shapes
    assert all(m['f64_dev'] < 1e-5 and 0.05 < m['y_absmax'] < 10 for m in metas)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_in_float32_matches_the_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = synth.lawfft_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x']
    x0 = x.clone()
    with torch.no_grad():
        y = O.lawfft_forward(sd, x)
    assert y.dtype == torch.float32 and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err, bar = (y - ref).abs().max().item(), bar_of(meta)
    print(f'MEASURE {name} oracle f32 against the fixture: {err:.3e} (bar {bar:.2e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= bar


@pytest.mark.parametrize('name', [n for n in NAMES if '_r4_' not in n])
def test_oracle_in_float64_transforms_in_float64(name):
    """In float64 the FFT form and the direct sum agree to 1e-12 through a whole model: nothing in between falls back to f32."""
    meta, arr = load_golden(name)
    sd = synth.lawfft_state_dict(seed=meta['seed'], **meta['synth'])
    with torch.no_grad():
        y = O.lawfft_forward(sd, arr['x'].double())
        yd = O.lawfft_forward(sd, arr['x'].double(), corr=O.corr_direct)
    assert y.dtype == torch.float64
    assert (y - yd).abs().max().item() <= 1e-12 * max(1.0, y.abs().max().item())
    assert (y - arr['y'].double()).abs().max().item() <= bar_of(meta)


@pytest.mark.parametrize('shape', [(2, 5, 8, 8), (1, 3, 16, 24), (1, 2, 9, 7)], ids=['8x8', '16x24', '9x7'])
def test_fft_form_against_the_direct_sum(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    q, k = torch.randn(shape, dtype=torch.float64, generator=gen), torch.randn(shape, dtype=torch.float64, generator=gen)
    a, b = O.corr_fft(q, k), O.corr_direct(q, k)
    assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()
    if shape[-1] % 2 == 0:  # the whole-image form as the model writes it: irfft2 without s= gives the map back at an even width
        assert torch.equal(a, torch.fft.irfft2(torch.fft.rfft2(q) * torch.fft.rfft2(k)))
    # the definition, element by element, at one place
    y, x = 3, 5 % shape[-1]
    H, W = shape[-2:]
    want = sum(q[0, 0, u, v] * k[0, 0, (y - u) % H, (x - v) % W] for u in range(H) for v in range(W))
    assert abs(b[0, 0, y, x] - want) <= 1e-12 * b.abs().max()
    if H % 8 == 0 and W % 8 == 0:  # per patch
        pa, pb = O.from_patches(O.corr_fft(O.to_patches(q), O.to_patches(k))), O.from_patches(O.corr_direct(O.to_patches(q), O.to_patches(k)))
        assert (pa - pb).abs().max().item() <= 1e-12 * pb.abs().max().item()
        assert torch.equal(pb[..., :8, :8], O.corr_direct(q[..., :8, :8], k[..., :8, :8]))


def test_the_synthetic_generators_have_live_and_dead_units():
    """The kernel-generating MLP's ReLU is active on some units and inactive on others, in both the narrow and the wide generators."""
    sd = synth.lawfft_state_dict(dim=32, local=8, n_rblock=1, n_mblock=2, scale=2, seed=1502)
    gen = torch.Generator().manual_seed(1)
    for p, c in (('body.0.residual.0.token_mix.1.local.0', 8), ('body.0.residual.0.token_mix.1.local.1', 8), ('body.0.residual.2', 32)):
        m = 0.5 * torch.randn(1, c, 1, 1, generator=gen)
        h = F.conv2d(m, sd[f'{p}.kernel_gen.1.weight'], sd[f'{p}.kernel_gen.1.bias'])
        assert (h > 0).any() and (h < 0).any(), p


def test_oracle_on_the_probe_sizes_the_reference_runs():
    meta, arr = load_golden('lawfft_probe')
    sd = synth.lawfft_state_dict(seed=meta['seed'], **meta['synth'])
    ran = [tuple(p['size']) for p in meta['probe'] if p['raises'] is None]
    assert set(ran) == {(5, 8), (8, 5), (8, 8), (9, 12)}
    for h, w in ran:
        with torch.no_grad():
            y = O.lawfft_forward(sd, arr[f'x_{h}x{w}'])
        ref = arr[f'y_{h}x{w}']
        assert y.shape == ref.shape and (y - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item()), (h, w)  # (no f64_dev recorded for the probe: the floor)
    for p in meta['probe']:
        if p['raises'] is not None:
            with pytest.raises(RuntimeError, match='Padding size should be less'):
                O.lawfft_forward(sd, torch.zeros(1, 3, *p['size']))
