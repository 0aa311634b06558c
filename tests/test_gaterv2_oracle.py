"""The CPU oracle of GateRv2 (tests/gaterv2_oracle.py: float64) against the reference's vectors (tools/gen_golden_gaterv2.py).  The bar is the
one tests/test_gaterv3_oracle.py uses (imported); the reference's own f32-against-f64 deviation on each case is printed beside it.  The probe
sizes the reference runs are held to the same bar, the oracle raises where the reference does, its x2 output's top-left corner is the
unmodified reference module's (cropped) output, and the attention formula alone is held to a literal einsum transcription within 1e-12."""

import pytest
import torch

import gaterv2_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth
from test_gaterv3_oracle import BAR

NAMES = [n for n in golden_names('gaterv2_') if n != 'gaterv2_probe']


def test_fixtures():
    assert len(NAMES) == 17 and all(load_golden(n)[0]['mode'] == 'eval' for n in NAMES)
    assert all(load_golden(n)[0]['scale_attribute_set'] == (load_golden(n)[0]['hyper']['scale'] != 1) for n in NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = synth.gaterv2_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].double()
    x0 = x.clone()
    with torch.no_grad():
        y = O.gaterv2_forward(sd, x)
    assert y.dtype == torch.float64 and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err = (y - ref.double()).abs().max().item()
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {BAR:.1e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= BAR


def test_oracle_on_the_probe_sizes():
    meta, arr = load_golden('gaterv2_probe')
    ran = 0
    for p in meta['probe']:
        sd = synth.gaterv2_state_dict(seed=meta['seed'], **meta['synth'][p['model']])
        h, w = p['size']
        if p['raises'] is None:
            key = f'x_{p["model"]}_{h}x{w}'
            if key not in arr:
                continue
            with torch.no_grad():
                y = O.gaterv2_forward(sd, arr[key].double())
            ref = arr[f'y_{p["model"]}_{h}x{w}']
            assert y.shape == ref.shape and (y - ref.double()).abs().max().item() <= BAR, (h, w)
            ran += 1
        else:
            assert p['raises'] == 'RuntimeError'
            with pytest.raises(RuntimeError, match='Padding size should be less than'):
                O.gaterv2_forward(sd, torch.rand(1, 3, h, w, dtype=torch.float64))
    assert ran >= 8


def test_oracle_raises_for_a_shorter_decoder():
    meta, _ = load_golden('gaterv2_probe')
    q = meta['dec_ne_enc']
    assert q['load']['raises'] is None and q['forward']['raises'] == 'RuntimeError' and 'channels' in q['forward']['message']
    sd = synth.gaterv2_state_dict(seed=meta['seed'], **q['synth'])
    with pytest.raises(RuntimeError, match='channels'):
        O.gaterv2_forward(sd, torch.rand(1, 3, 16, 16, dtype=torch.float64))


def test_the_unmodified_module_returns_the_top_left_corner():
    """``self.scale = 1`` in the reference module: its x2 output is the H x W corner of the full image."""
    meta, arr = load_golden('gaterv2_probe')
    q = meta['scale_crop']
    assert (q['scale_attribute'], q['scale_argument']) == (1, 2) and q['y_unmodified'] == q['x']
    case, carr = load_golden(q['case'])
    sd = synth.gaterv2_state_dict(seed=case['seed'], **case['synth'])
    assert torch.equal(arr['x_crop'], carr['x'])
    h, w = arr['x_crop'].shape[-2:]
    assert carr['y'].shape[-2:] == (2 * h, 2 * w) and torch.equal(carr['y'][:, :, :h, :w], arr['y_crop_unmodified'])
    with torch.no_grad():
        y = O.gaterv2_forward(sd, arr['x_crop'].double())
    assert (y[:, :, :h, :w] - arr['y_crop_unmodified'].double()).abs().max().item() <= BAR


@pytest.mark.parametrize('b,m,c,n', [(1, 1, 16, 1), (2, 2, 32, 6), (1, 6, 96, 129), (3, 48, 768, 7), (1, 64, 1024, 300)])
def test_the_attention_formula_against_a_literal_transcription(b, m, c, n):
    """``linear_attention`` against the formulae of the issue written as einsums, index for index, in f64."""
    g = torch.Generator().manual_seed(100 * m + n)
    q, k, v = (torch.randn(b, ch, n, generator=g, dtype=torch.float64) + 0.3 for ch in (m, m, c))
    qn = torch.einsum('bmn,bn->bmn', q, 1 / torch.sqrt(torch.einsum('bmn,bmn->bn', q, q)))
    kn = torch.einsum('bmn,bn->bmn', k, 1 / torch.sqrt(torch.einsum('bmn,bmn->bn', k, k)))
    ksum = torch.einsum('bmn->bm', kn) + 1e-6
    vsum = torch.einsum('bcn->bc', v)
    mat = torch.einsum('bmn,bcn->bmc', kn, v)
    t = 1 / (n + torch.einsum('bmn,bm->bn', qn, ksum))
    want = torch.einsum('bcn,bn->bcn', vsum[:, :, None] + torch.einsum('bmn,bmc->bcn', qn, mat), t)
    got = O.linear_attention(q, k, v)
    assert got.shape == (b, c, n)
    assert ((got - want).abs() / want.abs().clamp_min(1.0)).max().item() <= 1e-12
