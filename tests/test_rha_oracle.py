"""The plain-torch RHA oracle (tests/rha_oracle.py) pinned to every reference fixture on the CPU, and the synthetic checkpoints' statistics.

Bound: the oracle restates the reference's f32 arithmetic in another order of operations (the folded OmniShift kernel, one matrix product
per window batch), so it may differ from the fixture by about the reference's own f32-against-f64 deviation on the case, which every
fixture records as ``f64_dev`` (1.8e-7 .. 4.9e-7 at |y|max 0.36 .. 0.88).  In f32 the oracle must stay within 4 * f64_dev of the fixture; in
f64 within 2 * f64_dev (f64_dev itself is the distance of the fixture from the exact result, plus nothing of the oracle's)."""

import pytest
import torch

import rha_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('rha_')


def _sd(meta):
    kw = dict(meta['synth'])
    kw['down_list'] = tuple(kw['down_list'])
    return synth.rha_state_dict(seed=meta['seed'], **kw)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference(name):
    meta, arr = load_golden(name)
    sd = _sd(meta)
    x = arr['x'].clone()
    with torch.no_grad():
        y, y64 = O.rha_forward(sd, x), O.rha_forward(sd, x.double())
    assert torch.equal(x, arr['x'])  # the oracle leaves its input alone
    crop = meta.get('crop')
    if crop:
        assert list(y.shape) == meta['y_shape']
        y, y64 = y[:, :, : crop[1], : crop[3]], y64[:, :, : crop[1], : crop[3]]
    assert y.shape == arr['y'].shape
    e32, e64 = (y - arr['y']).abs().max().item(), (y64 - arr['y'].double()).abs().max().item()
    print(f'MEASURE {name}: f32 {e32:.3e}, f64 {e64:.3e} (f64_dev {meta["f64_dev"]:.3e})')
    assert e32 <= 4 * meta['f64_dev'] and e64 <= 2 * meta['f64_dev']


def test_hyper_parameters_read_back():
    meta, _ = load_golden('rha_x4_ps_d64_dn84_g2b2_40x70')
    hp = O.hyper(_sd(meta))
    assert (hp['dim'], hp['groups'], hp['res'], hp['down'], hp['hidden'], hp['head'], hp['scale'], hp['mid'], hp['ws']) == (64, 2, 2, [8, 4], 96, 'pixelshuffle', 4, 32, 8)


def test_synthetic_statistics_do_not_hide_the_blocks():
    sd = synth.rha_state_dict(dim=32, group_blocks=1, res_blocks=2, seed=5)
    for k, v in sd.items():
        if k.endswith('.bias'):
            assert bool((v != 0).all()), k
        elif k.endswith('.scale'):
            assert v.min() < -0.5 and v.max() > 0.5 and v.unique().numel() == v.numel()
        elif k.endswith('positional_encoding'):
            assert 0.4 < v.abs().max() <= 0.5
        elif 'alpha' in k:
            assert 0.75 <= v.min() and v.max() <= 1.25 and v.unique().numel() > 1
    k = 'body.0.body.0.conv.conv'
    assert not torch.allclose(sd[f'{k}.conv5x5_reparam.weight'], sd[f'{k}.conv5x5.weight'])  # the stored pair is not the fold: reading it shows
