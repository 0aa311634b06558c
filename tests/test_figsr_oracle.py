"""The CPU oracle of FIGSR (tests/figsr_oracle.py: float64, both transforms as dense matrix DFTs) against the reference's vectors
(tools/gen_golden_figsr.py), and the sizes of the probe fixture that the reference runs.

The bar is tied to each fixture's own ``f64_dev``, the deviation of the reference's f32 forward (what the fixture stores) from its forward
on a ``.double()`` copy:  2 * f64_dev + 2^-23 * max(1, |y|max).  The fixture is off from exact arithmetic by about f64_dev; the double
copy it was measured against still transforms in f32 (the module casts), a second contribution of the same order, hence the factor 2;
the last term is one f32 unit at the output's magnitude, for the rounding of the stored values themselves."""

import pytest
import torch

import figsr_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = [n for n in golden_names('figsr_') if n != 'figsr_probe']


def bar_of(meta) -> float:
    return 2.0 * meta['f64_dev'] + 2.0**-23 * max(1.0, meta['y_absmax'])


def test_fixtures_cover_what_the_issue_lists():
    metas = [load_golden(n)[0] for n in NAMES]
    hy = [m['hyper'] for m in metas]
    assert len(NAMES) == 11
    assert any((h['dim'], h['n_blocks'], h['scale'], h['upsampler']) == (48, 24, 4, 'pixelshuffledirect') for h in hy)
    assert {h['dim'] for h in hy} >= {32, 40, 48, 64} and {h['n_blocks'] for h in hy} >= {2, 3} and {h['gc'] for h in hy} == {8, 16}
    assert any((h['square_kernel_size'], h['band_kernel_size']) == (7, 11) for h in hy)
    assert {(h['upsampler'], h['scale']) for h in hy} >= {('conv', 1), ('pixelshuffledirect', 2), ('pixelshuffledirect', 4), ('pixelshuffle', 2), ('pixelshuffle', 3),
                                                          ('pixelshuffle', 4), ('nearest+conv', 3), ('nearest+conv', 4), ('dysample', 2), ('dysample', 3)}  # fmt: skip
    assert any('shift' in m['synth'] and 'scale_norm' in m['synth'] for m in metas)
    shapes = [tuple(load_golden(n)[1]['x'].shape) for n in NAMES]
    assert any(s[0] == 2 for s in shapes) and any(6 in s[2:] for s in shapes) and (1, 3, 9, 11) in shapes
    assert {(s[2] % 2, s[3] % 2) for s in shapes} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(m['f64_dev'] < 1e-6 and 0.1 < m['y_absmax'] < 10 for m in metas)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = synth.figsr_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].double()
    x0 = x.clone()
    with torch.no_grad():
        y = O.figsr_forward(sd, x)
    assert y.dtype == torch.float64 and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err, bar = (y - ref.double()).abs().max().item(), bar_of(meta)
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {bar:.2e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= bar


def test_oracle_on_the_probe_sizes_the_reference_runs():
    meta, arr = load_golden('figsr_probe')
    sd = synth.figsr_state_dict(seed=meta['seed'], **meta['synth'])
    ran = [tuple(p['size']) for p in meta['probe'] if p['raises'] is None]
    assert set(ran) == {(6, 6), (8, 9), (12, 7)}
    for h, w in ran:
        with torch.no_grad():
            y = O.figsr_forward(sd, arr[f'x_{h}x{w}'].double())
        ref = arr[f'y_{h}x{w}']
        assert y.shape == ref.shape and (y - ref.double()).abs().max().item() <= 1e-6, (h, w)  # (no f64_dev recorded for the probe: ten times the fixtures' largest)
    for p in meta['probe']:
        if p['raises'] is not None:
            with pytest.raises(RuntimeError, match='Padding size should be less'):
                O.figsr_forward(sd, torch.zeros(1, 3, *p['size'], dtype=torch.float64))
