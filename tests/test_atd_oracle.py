"""The plain-torch ATD oracle (tests/atd_oracle.py) pinned to the reference fixtures on the CPU (tools/gen_golden_atd.py).

With the reference's recorded permutations forced, the oracle reproduces ``y`` on every fixture.  Free-running (stable sort) it reproduces
the ids of the reference's stable run and ``y_stable`` on the guarded fixtures, whose smallest top-two margin is at least TAU; on the
others a rounding-level near-tie may legitimately flip, so they are not asserted free-running.  Tolerance 1e-5 * max(1, max|y|)."""

import pytest
import torch

import atd_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('atd_')


def _case(name):
    meta, arr = load_golden(name)
    kw = meta['synth']
    sd = synth.atd_state_dict(seed=meta['seed'], **kw)
    hyper = dict(window_size=kw['window_size'], category_size=meta['category_size'], upscale=kw['upscale'], upsampler=kw['upsampler'],
                 img_range=1.0, norm=kw.get('norm', True))  # fmt: skip
    return meta, arr, sd, hyper


def _crop(meta, y):
    crop = meta.get('crop')
    if crop:
        assert list(y.shape) == meta['y_shape']
        y = y[:, :, : crop[1], : crop[3]]
    return y


def test_fixture_coverage():
    metas = [load_golden(n)[0] for n in NAMES]
    assert sum(1 for m in metas if m['guarded']) >= 4
    assert all(m['min_margin'] >= O.TAU and m['decisions'] <= 3100 for m in metas if m['guarded'])
    assert {m['synth']['upsampler'] for m in metas} == {'', 'pixelshuffle', 'pixelshuffledirect', 'nearest+conv'}
    assert {m['synth']['window_size'] for m in metas} == {8, 16}
    assert {m['category_size'] for m in metas} == {128, 256}


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference_with_forced_permutations(name):
    meta, arr, sd, hyper = _case(name)
    force = [arr[f'perm_{li}'] for li in range(meta['layers'])]
    rec = {}
    with torch.no_grad():
        y = _crop(meta, O.atd_forward(sd, arr['x'], hyper, force=force, record=rec))
    assert y.shape == arr['y'].shape
    err = (y - arr['y']).abs().max().item()
    assert err <= 1e-5 * max(1.0, arr['y'].abs().max().item()), err
    if meta['guarded']:
        for li in range(meta['layers']):
            assert torch.equal(rec['ids'][li], arr[f'tk_id_{li}'].long())


@pytest.mark.parametrize('name', NAMES)
def test_oracle_free_running_on_guarded_fixtures(name):
    meta, arr, sd, hyper = _case(name)
    if not meta['guarded']:
        return  # a near-tie under TAU may flip between two float implementations: nothing to assert
    rec = {}
    with torch.no_grad():
        y = _crop(meta, O.atd_forward(sd, arr['x'], hyper, record=rec))
    for li in range(meta['layers']):
        assert torch.equal(rec['ids'][li], arr[f'tk_id_stable_{li}'].long()), li
        assert torch.equal(rec['perm'][li], torch.sort(rec['ids'][li], dim=-1, stable=True).indices)
    err = (y - arr['y_stable']).abs().max().item()
    assert err <= 1e-5 * max(1.0, arr['y_stable'].abs().max().item()), err


@pytest.mark.parametrize('name', NAMES)
def test_synth_keys_and_shapes_match_the_reference_module(name):
    meta, _ = load_golden(name)
    sd = synth.atd_state_dict(seed=meta['seed'], **meta['synth'])
    assert {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
