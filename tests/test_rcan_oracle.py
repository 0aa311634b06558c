"""The plain-torch RCAN oracle (tests/rcan_oracle.py) pinned to every reference fixture on the CPU, and the synthetic checkpoints' names
and shapes against the reference module's state_dict recorded in each fixture."""

import pytest
import torch

import rcan_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('rcan_')


def test_fixtures_exist():
    assert len(NAMES) >= 9


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference(name):
    meta, arr = load_golden(name)
    sd = synth.rcan_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].clone()
    with torch.no_grad():
        y = O.rcan_forward(sd, x)
    assert torch.equal(x, arr['x'])  # the oracle leaves its input alone
    crop = meta.get('crop')
    if crop:
        assert list(y.shape) == meta['y_shape']
        y = y[:, :, : crop[1], : crop[3]]
    assert y.shape == arr['y'].shape
    assert (y - arr['y']).abs().max().item() <= 1e-5 * max(1.0, arr['y'].abs().max().item())


@pytest.mark.parametrize('name', NAMES)
def test_synth_keys_and_shapes_match_the_reference_module(name):
    meta, _ = load_golden(name)
    sd = synth.rcan_state_dict(seed=meta['seed'], **meta['synth'])
    assert {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
    assert list(sd) == list(meta['state_dict'])
