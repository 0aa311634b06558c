"""The CPU oracle of MoESR (tests/moesr_oracle.py) against the reference's vectors (tools/gen_golden_moesr.py), in float32 and in float64.

The bar is the one this family's siblings have (test_newer_oracles_f64.py: mosr, mosrv2): 1e-5 * |y|max.  The oracle computes in the dtype
of its input and leaves the input alone."""

import pytest
import torch

import moesr_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('moesr_')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name, dtype):
    meta, arr = load_golden(name)
    sd = synth.moesr_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].to(dtype)
    x0 = x.clone()
    with torch.no_grad():
        y = O.moesr_forward(sd, x)
    assert y.dtype == dtype and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err, bar = (y.double() - ref.double()).abs().max().item(), 1e-5 * ref.abs().max().item()
    print(f'MEASURE {name} oracle {dtype} against the fixture: {err:.3e} (bar {bar:.3e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= bar


def test_oracle_pads_and_crops():
    """Odd both ways: the output is scale x the input, and equals the even-size run on the reflect-padded input cropped."""
    sd = synth.moesr_state_dict(dim=16, n_blocks=1, n_block=1, scale=2, seed=5)
    x = synth.synth_input((1, 3, 7, 9), 5)
    y = O.moesr_forward(sd, x)
    yp = O.moesr_forward(sd, torch.nn.functional.pad(x, (0, 1, 0, 1), 'reflect'))
    assert y.shape == (1, 3, 14, 18) and torch.equal(y, yp[:, :, :14, :18])
