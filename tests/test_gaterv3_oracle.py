"""The CPU oracle of GateRV3 (tests/gaterv3_oracle.py: float64, every Conv3XC unfolded) against the reference's eval-mode vectors
(tools/gen_golden_gaterv3.py).  The bar is the project's fixture bar, 2e-4 max-abs (tests/test_gfisr_oracle.py); the reference's own
f32-against-f64 deviation on each case is printed beside it.  The probe sizes the reference runs are held to the same bar, and the oracle
raises where the reference does: the reflect pad of a side that is too small, and a decoder with fewer levels than the encoder."""

import pytest
import torch

import gaterv3_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = [n for n in golden_names('gaterv3_') if n != 'gaterv3_probe']
BAR = 2e-4


def test_fixtures():
    assert len(NAMES) == 18 and all(load_golden(n)[0]['mode'] == 'eval' for n in NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = synth.gaterv3_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].double()
    x0 = x.clone()
    with torch.no_grad():
        y = O.gaterv3_forward(sd, x)
    assert y.dtype == torch.float64 and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err = (y - ref.double()).abs().max().item()
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {BAR:.1e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= BAR


def test_oracle_on_the_probe_sizes():
    meta, arr = load_golden('gaterv3_probe')
    ran = 0
    for p in meta['probe']:
        sd = synth.gaterv3_state_dict(seed=meta['seed'], **meta['synth'][p['model']])
        h, w = p['size']
        if p['raises'] is None:
            key = f'x_{p["model"]}_{h}x{w}'
            if key not in arr:
                continue
            with torch.no_grad():
                y = O.gaterv3_forward(sd, arr[key].double())
            ref = arr[f'y_{p["model"]}_{h}x{w}']
            assert y.shape == ref.shape and (y - ref.double()).abs().max().item() <= BAR, (h, w)
            ran += 1
        else:
            assert p['raises'] == 'RuntimeError'
            with pytest.raises(RuntimeError, match='Padding size should be less than'):
                O.gaterv3_forward(sd, torch.rand(1, 3, h, w, dtype=torch.float64))
    assert ran >= 8


def test_oracle_raises_for_a_shorter_decoder():
    meta, _ = load_golden('gaterv3_probe')
    q = meta['dec_ne_enc']
    assert q['load']['raises'] is None and q['forward']['raises'] == 'RuntimeError' and 'channels' in q['forward']['message']
    sd = synth.gaterv3_state_dict(seed=meta['seed'], **q['synth'])
    with pytest.raises(RuntimeError, match='channels'):
        O.gaterv3_forward(sd, torch.rand(1, 3, 8, 8, dtype=torch.float64))


def test_a_missing_gamma_means_ones():
    sd = synth.gaterv3_state_dict(dim=8, enc_blocks=(1,), dec_blocks=(1,), num_latent=1, span_blocks=1, with_gamma=False, seed=4)
    x = synth.synth_input((1, 3, 4, 6), 4).double()
    ones = dict(sd, gamma=torch.ones(1, 3, 1, 1))
    with torch.no_grad():
        assert 'gamma' not in sd and torch.equal(O.gaterv3_forward(sd, x), O.gaterv3_forward(ones, x))
