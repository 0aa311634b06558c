"""The CPU oracles of MoSR, MoSRv2, RGT, FDAT, OmniSR, ATD, RCAN, GateR, EIMN, RHA and FlexNet compute in the dtype of their arguments:
a float64 input (the oracle casts the state dict to it) gives a float64 output, through ``helpers.oracle_forward``.

Every fixture of every family is run in float64 and compared with the reference's (float32) ``y`` at the bar the family's own float32
oracle test applies -- no new number:

    mosr, mosrv2, eimn     1e-5 * |y|max                (test_mosr_loader.py, test_eimn_oracle.py)
    rgt                    2e-5 * max(1, |y|max)        (test_rgt_loader.py)
    fdat, omnisr, rcan     1e-5 * max(1, |y|max)        (test_<arch>_oracle.py)
    atd                    1e-5 * max(1, |y|max), the reference's recorded permutations forced (test_atd_oracle.py)
    gater                  test_gater_oracle.TOL
    rha, flexnet           2 * the fixture's f64_dev    (test_rha_oracle.py, test_flexnet_oracle.py)

A float32 fixture is at its own rounding distance from the exact result, so the float64 run cannot be asked for less than that.
"""

import pytest
import torch

from helpers import golden_names, load_golden, oracle_forward
from resselt_amd.utils import synth
from test_gater_oracle import TOL as GATER_TOL

FAMILIES = ('mosr', 'mosrv2', 'rgt', 'fdat', 'omnisr', 'atd', 'rcan', 'gater', 'eimn', 'rha', 'flexnet')
CASES = [(f, n) for f in FAMILIES for n in golden_names(f + '_')]


def _bar(family, meta, y):
    top = y.abs().max().item()
    if family in ('mosr', 'mosrv2', 'eimn'):
        return 1e-5 * top
    if family == 'rgt':
        return 2e-5 * max(1.0, top)
    if family == 'gater':
        return GATER_TOL
    if family in ('rha', 'flexnet'):
        return 2 * meta['f64_dev']
    return 1e-5 * max(1.0, top)


def oracle_meta(family, meta, arr=None):
    """What ``helpers.oracle_forward`` needs for a fixture's ``meta``."""
    kw = meta['synth']
    om = dict(arch=family)
    if family == 'mosr':
        om.update(upsampler=kw.get('upsampler', 'ps'), upscale=meta['metadata']['upscale'])
    elif family == 'mosrv2':
        om.update(upsampler=kw.get('upsampler', 'pixelshuffledirect'), upscale=meta['metadata']['upscale'], mid_dim=kw.get('mid_dim', 32))
    elif family == 'rgt':
        om.update(split_size=kw['split_size'], num_heads=kw['num_heads'], c_ratio=kw.get('c_ratio', 0.5))
    elif family == 'atd':
        om['hyper'] = dict(window_size=kw['window_size'], category_size=meta['category_size'], upscale=kw['upscale'], upsampler=kw['upsampler'],
                           img_range=1.0, norm=kw.get('norm', True))  # fmt: skip
        if arr is not None:
            om['force'] = [arr[f'perm_{li}'] for li in range(meta['layers'])]
    return om


def test_every_family_has_fixtures():
    assert {f for f, _ in CASES} == set(FAMILIES)


@pytest.mark.parametrize('family,name', CASES)
def test_float64_oracle_matches_fixture(family, name):
    meta, arr = load_golden(name)
    kw = {k: tuple(v) if isinstance(v, list) else v for k, v in meta['synth'].items()}
    sd = getattr(synth, f'{family}_state_dict')(seed=meta['seed'], **kw)
    x = (arr['x'] if 'x' in arr else arr['x_u8'].float() / 255).double()
    x0 = x.clone()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    with torch.no_grad():
        y = oracle_forward(oracle_meta(family, meta, arr), sd64, x)
        y_mixed = oracle_forward(oracle_meta(family, meta, arr), sd, x)  # a float32 state dict follows the input's dtype too
    assert y.dtype == torch.float64 and y_mixed.dtype == torch.float64
    assert torch.equal(y, y_mixed)
    assert torch.equal(x, x0)  # the oracle leaves its input alone
    if 'y_crop' in arr:
        c = meta['crop']
        y, ref = y[:, :, c[0] : c[1], c[2] : c[3]], arr['y_crop']
    else:
        ref = arr['y']
        crop = meta.get('crop')
        if crop:
            assert list(y.shape) == meta['y_shape']
            y = y[:, :, : crop[1], : crop[3]]
    assert y.shape == ref.shape
    err, bar = (y - ref.double()).abs().max().item(), _bar(family, meta, ref)
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {bar:.3e})')
    assert err <= bar
