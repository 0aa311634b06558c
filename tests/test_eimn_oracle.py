"""The plain-torch EIMN oracle (tests/eimn_oracle.py) pinned to every reference fixture on the CPU, and the synthetic checkpoints' names
and shapes against the reference module's state_dict recorded in each fixture."""

import pytest
import torch

import eimn_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('eimn_')


def test_fixtures_exist():
    assert len(NAMES) == 6
    metas = [load_golden(n)[0] for n in NAMES]
    assert all(m['mode'] == 'eval' and m['claimed_by'] == 'eimn' for m in metas)
    assert {m['hyper']['hidden'] for m in metas} == {170, 127, 128}
    assert [18, 6, 24] in [m['hyper']['splits'] for m in metas] and 16 in {m['hyper']['num_stages'] for m in metas}


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference(name):
    meta, arr = load_golden(name)
    sd = synth.eimn_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].clone()
    with torch.no_grad():
        y = O.eimn_forward(sd, x)
    assert torch.equal(x, arr['x'])  # the oracle leaves its input alone
    crop = meta.get('crop')
    if crop:
        assert list(y.shape) == meta['y_shape']
        y = y[:, :, : crop[1], : crop[3]]
    assert y.shape == arr['y'].shape
    assert (y - arr['y']).abs().max().item() <= 1e-5 * arr['y'].abs().max().item()


@pytest.mark.parametrize('name', NAMES)
def test_synth_keys_and_shapes_match_the_reference_module(name):
    meta, _ = load_golden(name)
    sd = synth.eimn_state_dict(seed=meta['seed'], **meta['synth'])
    assert {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
    assert list(sd) == list(meta['state_dict'])


def test_synthetic_statistics_do_not_hide_the_blocks():
    sd = synth.eimn_state_dict(seed=5)
    for k, v in sd.items():
        if k.endswith('running_var'):
            assert 0.5 <= v.min() and v.max() <= 1.5
        elif k.endswith('running_mean'):
            assert 0.15 < v.abs().max() <= 0.3
        elif 'layer_scale' in k:
            assert 0.1 <= v.min() and v.max() <= 0.6
        elif k.endswith('.bias'):
            assert bool((v != 0).all()), k
