"""The CPU oracles under oracle/ (RRDBNet, SPAN, SPANPlus, SpanPP, Compact, RTMoSR, SwinIR, DAT, HAT, DRCT, PLKSR / RealPLKSR, Real-CUGAN)
compute in the dtype of their arguments: a float64 state dict and a float64 input give a float64 output, through ``helpers.oracle_forward``.

Every fixture test_oracle_golden.py replays is run in float64 and compared with the reference's (float32) ``y`` at that file's bar,
1e-5 * max(1, |y|max) -- no new number.  A float32 fixture is at its own rounding distance from the exact result, so the float64 run
cannot be asked for less than that.  The GPU sweeps (test_original_archs_sweep_gpu.py, test_plksr_cugan_sweep_gpu.py) compare with these
float64 runs.
"""

import pytest
import torch

from helpers import load_golden, oracle_forward, synth_state_dict
from test_oracle_golden import E2E

FAMILIES = ('rrdbnet', 'span', 'spanplus', 'spanpp', 'compact', 'rtmosr', 'swinir', 'dat', 'hat', 'drct', 'plksr', 'realplksr', 'cugan')


def test_every_family_has_fixtures():
    assert {n.split('_')[0] for n in E2E} == set(FAMILIES)


@pytest.mark.parametrize('name', E2E)
def test_float64_oracle_matches_fixture(name):
    meta, arr = load_golden(name)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in synth_state_dict(meta).items()}
    x = arr['x'].double()
    x0 = x.clone()
    with torch.no_grad():
        y = oracle_forward(meta, sd64, x)
    assert y.dtype == torch.float64
    assert torch.equal(x, x0)  # the oracle leaves its input alone
    ref = arr['y']
    assert y.shape == ref.shape
    err, bar = (y - ref.double()).abs().max().item(), 1e-5 * max(ref.abs().max().item(), 1.0)
    print(f'MEASURE {name} oracle f64 against the fixture: {err:.3e} (bar {bar:.3e})')
    assert err <= bar
