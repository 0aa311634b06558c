"""Whole-model GPU sweep of GFISR v1 over input sizes, on tests/sweep_common.py: every side from 4 to 13 on each axis beside an even and
an odd other side (the FourierUnit pads an odd side by one more row / column, and the DFT tables are per padded size), batch 1 and 2,
against the float64 oracle (tests/gfisr_oracle.py), for one small model: dim 16, 5 blocks (every rotation of the five Inception modules),
x2, no unshuffle.  Every case runs twice, the second run bit-equal.  Tolerance (asserted): sweep_common.FUZZ_BAR; the family bar
(test_gfisrv2_gpu.MODEL_REL) is printed beside it.  Below the swept range the oracle and the engine refuse the same sizes."""

import pytest
import torch

import gfisr_oracle as O
from sweep_common import Case as _Case
from sweep_common import _check, _input, _status_ok  # noqa: F401  (the fixture checks the status word after every test)
from test_gfisrv2_gpu import MODEL_REL

pytestmark = pytest.mark.gpu

SIDES = range(4, 14)
SHAPES = sorted({hw for s in SIDES for hw in ((s, 6), (s, 7), (6, s), (7, s))})


class Case(_Case):
    configs = {'gfisr': ('gfisr', dict(scale=2, dim=16, n_blocks=5), 0, 13, 6)}
    family_bar = {'gfisr': lambda ref: MODEL_REL * max(1.0, ref.abs().max().item())}

    def oracle(self, x, f64=True):
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            return O.gfisr_forward(self.sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        try:
            self.oracle(torch.rand(1, self.cin, h, w))
        except RuntimeError:  # the FourierUnit's reflect pad
            return False
        return True


_cases: dict = {}


def _case(device):
    if 'gfisr' not in _cases:
        _cases['gfisr'] = Case('gfisr', device)
    return _cases['gfisr']


def test_the_sweep_covers_both_parities_on_each_axis():
    assert len(SHAPES) == 36
    for axis in (0, 1):
        for s in SIDES:
            assert {hw[1 - axis] % 2 for hw in SHAPES if hw[axis] == s} == {0, 1}
    assert {1 + (h + w) % 2 for h, w in SHAPES} == {1, 2}


@pytest.mark.parametrize('hw', SHAPES, ids=[f'{h}x{w}' for h, w in SHAPES])
def test_sizes(device, hw):
    c = _case(device)
    n = 1 + (hw[0] + hw[1]) % 2  # batch 1 and 2, each with every side on each axis
    _check(c, _input(c, (n, c.cin, *hw), seed=100 * hw[0] + hw[1]), device, what='sweep')


def test_sizes_below_the_range_are_refused_like_the_oracle(device):
    c = _case(device)
    for h, w in ((3, 6), (6, 3), (3, 3), (2, 7), (7, 1)):
        assert not c.accepts(h, w)
        with pytest.raises(RuntimeError, match='Padding size should be less than'):
            c.run(torch.rand(1, c.cin, h, w, device=device))
    assert c.accepts(4, 4) and c.accepts(4, 5) and c.accepts(5, 4)
    _check(c, _input(c, (1, c.cin, 4, 5), seed=7), device, what='after the refusals')
