"""The plain-torch GateR oracle (tests/gater_oracle.py) pinned to every reference fixture on the CPU in f32.

Tolerance.  The reference's own f32-against-f64 deviation on these fixtures is 1.9e-7 .. 8.1e-7 at |y|max 1.18 .. 1.52 (recorded in each
fixture as ``f64_dev`` / ``y_absmax``; the synthetic checkpoints scale the last convolution by 0.1, so the outputs sit near the image range).
Measured oracle-against-fixture deviation with these weights, f32: 1.6e-7 .. 7.7e-7 (largest: gater_d24_att_n2_13x18).  Pinned at twice the
largest: 1.6e-6.  In f64 the oracle reproduces the reference's f64 result to the fixture's own f32 error, which bounds that run by the same
figure."""

import pytest
import torch

import gater_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.utils import synth

NAMES = golden_names('gater_')
TOL = 1.6e-6


def _run(name, dtype):
    meta, arr = load_golden(name)
    sd = synth.gater_state_dict(seed=meta['seed'], **meta['synth'])
    x = arr['x'].clone()
    with torch.no_grad():
        y = O.gater_forward(sd, x.to(dtype))
    assert torch.equal(x, arr['x'])  # the oracle leaves its input alone
    assert list(y.shape) == meta['y_shape']
    crop = meta.get('crop')
    if crop:
        y = y[:, :, : crop[1], : crop[3]]
    return meta, (y.double() - arr['y'].double()).abs().max().item()


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference_f32(name):
    meta, dev = _run(name, torch.float32)
    print(f'MEASURE {name} oracle f32 dev {dev:.3e} |y|max {meta["y_absmax"]:.3f} reference f32-f64 {meta["f64_dev"]:.3e}')
    assert dev <= TOL


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference_f64(name):
    meta, dev = _run(name, torch.float64)
    assert dev <= TOL
    assert abs(dev - meta['f64_dev']) <= 1e-7  # the f64 oracle IS the reference's f64 run: what is left is the fixture's f32 error
