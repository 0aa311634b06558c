"""The CPU oracle of GFISRv2 (tests/gfisrv2_oracle.py: float64, both transforms as dense matrix DFTs) against the reference's vectors
(tools/gen_golden_gfisrv2.py).  The bar is the project's fixture bar, 2e-4 max-abs; the reference's own f32-against-f64 deviation on each
case is printed beside it.  The tiny inputs the reference runs (1x2, 2x1, 1x3, 3x1) are held to the same bar."""

import pytest
import torch

import gfisrv2_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = [n for n in golden_names('gfisrv2_') if n != 'gfisrv2_tiny_probe']
BAR = 2e-4


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = synth.gfisrv2_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].double()
    x0 = x.clone()
    with torch.no_grad():
        y = O.gfisrv2_forward(sd, x)
    assert y.dtype == torch.float64 and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err = (y - ref.double()).abs().max().item()
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {BAR:.1e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= BAR


def test_oracle_on_the_tiny_inputs_the_reference_runs():
    meta, arr = load_golden('gfisrv2_tiny_probe')
    sd = synth.gfisrv2_state_dict(seed=meta['seed'], **meta['synth'])
    ran = [tuple(p['size']) for p in meta['probe'] if p['raises'] is None]
    assert ran
    for h, w in ran:
        with torch.no_grad():
            y = O.gfisrv2_forward(sd, arr[f'x_{h}x{w}'].double())
        ref = arr[f'y_{h}x{w}']
        assert y.shape == ref.shape and (y - ref.double()).abs().max().item() <= BAR, (h, w)
