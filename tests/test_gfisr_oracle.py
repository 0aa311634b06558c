"""The CPU oracle of GFISR v1 (tests/gfisr_oracle.py: float64, both transforms as dense matrix DFTs around an explicit reflect pad and
crop) against the reference's vectors (tools/gen_golden_gfisr.py).  The bar is the project's fixture bar, 2e-4 max-abs; the reference's own
f32-against-f64 deviation on each case is printed beside it.  The probe sizes the reference runs (4x4, 4x5, 5x5) are held to the same bar,
and the oracle raises where the reference's reflect pad does."""

import pytest
import torch

import gfisr_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = [n for n in golden_names('gfisr_') if n != 'gfisr_probe']
BAR = 2e-4


def test_fixtures():
    assert len(NAMES) == 12 and sum(load_golden(n)[0]['direct'] for n in NAMES) == 2


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = synth.gfisr_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].double()
    x0 = x.clone()
    with torch.no_grad():
        y = O.gfisr_forward(sd, x, scale=meta['hyper']['scale'])
    assert y.dtype == torch.float64 and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err = (y - ref.double()).abs().max().item()
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {BAR:.1e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= BAR


def test_oracle_on_the_probe_sizes():
    meta, arr = load_golden('gfisr_probe')
    sd = synth.gfisr_state_dict(seed=meta['seed'], **meta['synth'])
    probe = {tuple(p['size']): p['raises'] for p in meta['probe']}
    assert set(probe) == {(3, 3), (3, 4), (4, 3), (4, 4), (4, 5), (5, 5)}
    for (h, w), raises in probe.items():
        if raises is None:
            with torch.no_grad():
                y = O.gfisr_forward(sd, arr[f'x_{h}x{w}'].double())
            ref = arr[f'y_{h}x{w}']
            assert y.shape == ref.shape and (y - ref.double()).abs().max().item() <= BAR, (h, w)
        else:
            assert raises == 'RuntimeError'
            with pytest.raises(RuntimeError, match='Padding size should be less than'):
                O.gfisr_forward(sd, torch.rand(1, 3, h, w, dtype=torch.float64))
