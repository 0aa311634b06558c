"""The CPU oracles of MoSR, MoSRv2, RGT, FDAT, OmniSR, ATD, RCAN, GateR, EIMN, RHA, FlexNet, MoESR, SMoSR and GFISRv2 compute in the
dtype of their arguments: a float64 input (the oracle casts the state dict to it) gives a float64 output, through ``helpers.oracle_forward``.

Every fixture of every family is run in float64 and compared with the reference's (float32) ``y`` at the bar the family's own float32
oracle test applies -- no new number:

    mosr, mosrv2, eimn     1e-5 * |y|max                (test_mosr_loader.py, test_eimn_oracle.py)
    moesr, smosr           1e-5 * |y|max                (test_moesr_oracle.py, test_smosr_oracle.py)
    gfisrv2                test_gfisrv2_oracle.BAR, the tiny probe's four inputs included
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
from test_gfisrv2_oracle import BAR as GFISRV2_BAR

FAMILIES = ('mosr', 'mosrv2', 'rgt', 'fdat', 'omnisr', 'atd', 'rcan', 'gater', 'eimn', 'rha', 'flexnet', 'moesr', 'smosr', 'gfisrv2')
CASES = [(f, n) for f in FAMILIES for n in golden_names(f + '_')]


def _bar(family, meta, y):
    top = y.abs().max().item()
    if family in ('mosr', 'mosrv2', 'eimn', 'moesr', 'smosr'):
        return 1e-5 * top
    if family == 'gfisrv2':
        return GFISRV2_BAR
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
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    # (GFISRv2's probe fixture holds the four tiny inputs the reference runs instead of one ``x``)
    pairs = [(f'x_{h}x{w}', f'y_{h}x{w}') for h, w in (p['size'] for p in meta['probe']) if f'x_{h}x{w}' in arr] if 'probe' in meta else [(None, 'y')]
    assert pairs
    for xk, yk in pairs:
        _one(family, name, meta, arr, sd, sd64, xk, yk)


def _one(family, name, meta, arr, sd, sd64, xk, yk):
    x = (arr[xk] if xk else arr['x'] if 'x' in arr else arr['x_u8'].float() / 255).double()
    x0 = x.clone()
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
        ref = arr[yk]
        crop = meta.get('crop')
        if crop:
            assert list(y.shape) == meta['y_shape']
            y = y[:, :, : crop[1], : crop[3]]
    assert y.shape == ref.shape
    err, bar = (y - ref.double()).abs().max().item(), _bar(family, meta, ref)
    print(f'MEASURE {name}{" " + xk if xk else ""} oracle f64 against the fixture: {err:.3e} (bar {bar:.3e})')
    assert err <= bar
