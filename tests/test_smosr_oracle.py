"""The CPU oracle of SMoSR (tests/smosr_oracle.py) against the reference's vectors (tools/gen_golden_smosr.py), in float32 and in float64,
and the conditions every fixture must meet so that the bars of the GPU tests cannot hide a failure.

The bar is the one this family's siblings have (test_moesr_oracle.py, test_newer_oracles_f64.py): 1e-5 * |y|max.  The oracle computes in
the dtype of its input and leaves the input alone."""

import pytest
import torch

import smosr_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('smosr_')


def test_fixtures_cover_the_issue_and_are_conditioned():
    assert len(NAMES) == 14
    metas = {n: load_golden(n)[0] for n in NAMES}
    hy = [m['hyper'] for m in metas.values()]
    assert {h['upsampler'] for h in hy} == {'conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'pa_up'}
    assert {(h['upsampler'], h['scale'], h['rep']) for h in hy} >= {
        ('pixelshuffledirect', 2, 0), ('pixelshuffledirect', 2, 1), ('pa_up', 4, 1), ('pa_up', 3, 0), ('pixelshuffle', 3, 0), ('nearest+conv', 4, 0),
        ('nearest+conv', 2, 1), ('dysample', 2, 0), ('conv', 1, 0)}  # fmt: skip
    assert {h['d_kernel'] for h in hy if h['upsampler'] == 'dysample'} == {1, 3}
    assert any(h['in_ch'] == 1 and h['out_ch'] == 1 and h['dim'] == 24 for h in hy)
    # hidden head widths that are no whole planes / whose DySample groups are no whole units of four channels
    assert {(h['upsampler'], h['upsampler_mid_dim'], h['d_kernel']) for h in hy} >= {('pixelshuffle', 20, 1), ('dysample', 12, 1), ('dysample', 20, 3)}
    for name, m in metas.items():
        print(f"MEASURE {name}: |y|max {m['y_absmax']:.3f}  f64_dev {m['f64_dev']:.2e}  gate median {m['gate_median']:.3f}  above 3: {m['gate_above3']:.5f}")
        assert m['y_absmax'] >= 0.5, name
        assert m['f64_dev'] <= 1e-5 * m['y_absmax'], name
        assert 0.05 <= m['gate_median'] <= 2 and m['gate_above3'] < 0.01, name
        assert m['claimed_by'] == 'SMoSR' and m['claims'] == ['SMoSR'], name  # in the reference's registry too


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_the_reference_vectors(name, dtype):
    meta, arr = load_golden(name)
    sd = synth.smosr_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].to(dtype)
    x0 = x.clone()
    with torch.no_grad():
        y = O.smosr_forward(sd, x)
    assert y.dtype == dtype and torch.equal(x, x0)
    ref = arr['y']
    assert y.shape == ref.shape
    err, bar = (y.double() - ref.double()).abs().max().item(), 1e-5 * ref.abs().max().item()
    print(f'MEASURE {name} oracle {dtype} against the fixture: {err:.3e} (bar {bar:.3e}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= bar


def test_oracle_pads_and_crops():
    """Odd both ways: the output is scale x the input, and equals the body of the network (no pad, no crop) on the input reflect-padded by
    2 on all four sides, cropped by 2 * scale on all four sides."""
    sd = synth.smosr_state_dict(dim=16, n_mb=1, seed=5)
    x = synth.synth_input((1, 3, 7, 9), 5).double()
    y = O.smosr_forward(sd, x)
    assert y.shape == (1, 3, 14, 18)
    xp = torch.nn.functional.pad(x, (2, 2, 2, 2), 'reflect')
    sdd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    full = O.head(_plain(sdd), _features(sdd, xp), 'pixelshuffledirect', 2)
    assert torch.equal(y, full[:, :, 4:-4, 4:-4])


def _plain(sd):
    return {k: v for k, v in sd.items() if not k.endswith('MetaUpsample')}


def _features(sd, xp):
    """cat[s, f] of an ALREADY padded input (the body of smosr_forward without its pad and crop)."""
    sd = _plain(sd)
    s = torch.nn.functional.conv2d(xp, sd['short.weight'], sd['short.bias'])
    f = O.smb(sd, 'blocks_1.1', O.smb(sd, 'blocks_1.0', xp))
    t = O.smb(sd, 'blocks_2.0', f)
    f = O.conv(sd, 'end_block.1', O.smb(sd, 'end_block.0', t + f))
    return torch.cat([s, f], 1)
