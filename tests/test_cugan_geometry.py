"""Real-CUGAN's plan geometry against the oracle (oracle/cugan.py), without a GPU.

* Shapes: the oracle runs on the ``meta`` device, where a reflect pad that is too large and mismatched U-Net maps raise just as they do on
  real tensors, so every input size costs only its shape arithmetic.  For h0 and w0 over 1..96 (one side at a time, the other fixed at a
  legal size of the other parity, plus the diagonal), ``cugan_layers`` must refuse exactly the sizes the oracle refuses and, otherwise,
  promise the oracle's output size.  This generalises test_cugan_loader.test_minimum_sizes_match_reference.
* Values: the float64 replay of the plan's layer records (test_cugan_loader.replay -- the windows, origins, crops and phases the kernels
  use) equals the float64 oracle at eight consecutive legal heights per variant, so a window that is the right size at the wrong place
  fails here at some residue, not only at the fixture sizes.
"""

import pytest
import torch

from oracle.cugan import cugan_forward
from resselt_amd.archs.cugan.arch import VARIANTS, cugan_layers
from resselt_amd.utils import synth
from test_cugan_loader import replay

SIDES = range(1, 97)
# a legal size per variant of each parity (the 2x_fast sides that work are 0 or 3 mod 4, from 40 up)
FIXED = {'2x': (24, 25), '3x': (24, 21), '4x': (24, 25), '2x_fast': (44, 43)}


def _oracle_hw(sd, h0, w0):
    try:
        y = cugan_forward(sd, torch.empty((1, 3, h0, w0), device='meta'))
    except RuntimeError:
        return None
    return tuple(y.shape[2:])


def _plan_hw(variant, h0, w0):
    try:
        return cugan_layers(variant, 3, 3, h0, w0).out_hw
    except ValueError:
        return None


@pytest.mark.parametrize('variant', VARIANTS)
def test_plan_refuses_and_sizes_as_the_oracle(variant):
    sd = {k: v.to('meta') for k, v in synth.cugan_state_dict(variant).items()}
    even, odd = FIXED[variant]
    sizes = [(h, odd) for h in SIDES] + [(even, w) for w in SIDES] + [(s, s) for s in SIDES]
    legal = 0
    for h0, w0 in sizes:
        want = _oracle_hw(sd, h0, w0)
        assert _plan_hw(variant, h0, w0) == want, f'{variant} {h0}x{w0}: the oracle gives {want}'
        legal += want is not None
    assert 0 < legal < len(sizes)  # both sides of the boundary were reached


def _legal_heights(variant, w0, count=8):
    """The smallest ``count`` consecutive heights that are legal with width w0 (for 2x_fast: the legal heights from the minimum up)."""
    hs = [h for h in range(1, 120) if _plan_hw(variant, h, w0) is not None]
    return hs[:count]


@pytest.mark.parametrize('variant, pro', [('2x', False), ('2x', True), ('3x', False), ('3x', True), ('4x', False), ('4x', True), ('2x_fast', False)])
def test_plan_replay_matches_oracle_across_residues(variant, pro):
    sd = synth.cugan_state_dict(variant, pro=pro, seed=11)
    sd64 = {k: v.to(torch.float64) for k, v in sd.items()}
    w0 = FIXED[variant][1] + (4 if variant == '2x_fast' else 2)  # the odd legal width, two (2x_fast: four) above the fixed one
    hs = _legal_heights(variant, w0)
    assert len(hs) == 8
    for h0 in hs:
        x = synth.synth_input((1, 3, h0, w0), seed=h0)
        with torch.no_grad():
            want = cugan_forward(sd64, x.to(torch.float64))
            got = replay(variant, sd, x, pro)
        assert got.shape == want.shape, f'{variant} {h0}x{w0}'
        err = (got - want).abs().max().item()
        assert err <= 1e-9 * max(1.0, want.abs().max().item()), f'{variant} pro={pro} {h0}x{w0}: max-abs {err:.3e}'
