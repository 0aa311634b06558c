"""The plain-torch FlexNet oracle (tests/flexnet_oracle.py) pinned to every reference fixture on the CPU, and the synthetic checkpoints'
statistics.

Bound (the acceptance rule of tests/test_rha_oracle.py): the oracle restates the reference's f32 arithmetic in another order of operations
(the folded OmniShift kernel, one matrix product per window batch), so it may differ from the fixture by about the reference's own
f32-against-f64 deviation on the case, which every fixture records as ``f64_dev`` (1.1e-7 .. 5.0e-7 at |y|max 0.23 .. 0.95).  In f32 the
oracle must stay within 4 * f64_dev of the fixture; in f64 within 2 * f64_dev (f64_dev itself is the distance of the fixture from the exact
result, plus nothing of the oracle's).  The oracle's RMSNorm eps is 2^-23 in either dtype, as the fixtures' f64 run."""

import pytest
import torch

import flexnet_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('flexnet_')


def _sd(meta):
    kw = dict(meta['synth'])
    kw['num_blocks'] = tuple(kw['num_blocks'])
    return synth.flexnet_state_dict(seed=meta['seed'], **kw)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference(name):
    meta, arr = load_golden(name)
    sd = _sd(meta)
    x = arr['x'].clone()
    with torch.no_grad():
        y, y64 = O.flexnet_forward(sd, x), O.flexnet_forward(sd, x.double())
    assert torch.equal(x, arr['x'])  # the oracle leaves its input alone
    crop = meta.get('crop')
    if crop:
        assert list(y.shape) == meta['y_shape']
        y, y64 = y[:, :, : crop[1], : crop[3]], y64[:, :, : crop[1], : crop[3]]
    assert y.shape == arr['y'].shape and y.dtype == torch.float32 and y64.dtype == torch.float64
    e32, e64 = (y - arr['y']).abs().max().item(), (y64 - arr['y'].double()).abs().max().item()
    print(f'MEASURE {name}: f32 {e32:.3e}, f64 {e64:.3e} (f64_dev {meta["f64_dev"]:.3e})')
    assert e32 <= 4 * meta['f64_dev'] and e64 <= 2 * meta['f64_dev']


def test_hyper_parameters_read_back():
    meta, _ = load_golden('flexnet_x3_dys_d48_b31_cn_n2_9x11')
    hp = O.hyper(_sd(meta))
    assert (hp['dim'], hp['blocks'], hp['hidden'], hp['hidden_rate'], hp['head'], hp['scale'], hp['channel_norm'], hp['window']) == (48, [3, 1], 192, 4, 'dys', 3, True, 8)
    hp = O.hyper(_sd(load_golden('flexnet_x4_nc_d16_gray_hr2_9x20')[0]))
    assert (hp['dim'], hp['in_ch'], hp['out_ch'], hp['hidden_rate'], hp['head'], hp['scale']) == (16, 1, 1, 2, 'n+c', 4)


def test_the_stored_reparam_weight_is_ignored_and_eps_matters():
    meta, arr = load_golden('flexnet_x4_nc_d16_gray_hr2_9x20')
    sd = _sd(meta)
    other = {k: (torch.full_like(v, 7.0) if 'conv5x5_reparam' in k else v) for k, v in sd.items()}
    with torch.no_grad():
        assert torch.equal(O.flexnet_forward(sd, arr['x']), O.flexnet_forward(other, arr['x']))
        x = torch.zeros(1, 16, 8, 8, dtype=torch.float64)
        x[0, :, 0, 0] = 1e-4
        n = O.rmsnorm(x, torch.ones(16))
    assert float(n[0, 0, 1, 1]) == 0.0  # a pixel of zeros gives zeros
    assert abs(float(n[0, 0, 0, 0]) - 1e-4 / (1e-8 + 2.0**-23) ** 0.5) < 1e-12 and float(n[0, 0, 0, 0]) < 0.3  # eps 2^-23 in f64 too, and it matters at 1e-4


def test_synthetic_statistics_do_not_hide_the_blocks():
    sd = synth.flexnet_state_dict(dim=32, num_blocks=(2,), seed=5, channel_norm=True)
    for k, v in sd.items():
        if k.endswith('.bias'):
            assert bool((v != 0).all()), k
        elif k.endswith('gamma1') or k.endswith('gamma2'):
            assert 0.1 <= v.min() and v.max() <= 0.3 and v.unique().numel() == v.numel()
        elif k.endswith('.alpha'):
            assert v.shape == (4,) and 0.19 <= v.min() and v.max() <= 0.31 and v.unique().numel() == 4
        elif k.endswith('rn1.weight') or k.endswith('key_norm.weight'):
            assert 0.5 <= v.min() and v.max() <= 1.5 and v.unique().numel() > 1
    k = 'pipeline.att.0.t_blocks.0.att.omni_shift'
    assert not torch.allclose(sd[f'{k}.conv5x5_reparam.weight'], sd[f'{k}.conv5x5.weight'])  # the stored weight is not the fold: reading it shows
    assert sd['window_size'].dtype == torch.uint8 and int(sd['window_size']) == 8
    assert torch.equal(synth.flexnet_state_dict(dim=16, num_blocks=(1,), seed=2)['in_to_feat.weight'], synth.flexnet_state_dict(dim=16, num_blocks=(1,), seed=2)['in_to_feat.weight'])
