"""A short whole-model GPU sweep of GateRv2 over input sizes, on tests/sweep_common.py, against the float64 oracle
(tests/gaterv2_oracle.py): every side from 1 to 2 P + 1 on either axis for a two-level x2 model (P = 4), acceptance exactly where the
oracle raises, a batch of three with different statistics per image (sca's mean and the attention are per image), and one frame with more
than one reduction tile and more than one token chunk.  Every case runs twice, the second run bit-equal.  Tolerance (asserted):
sweep_common.FUZZ_BAR, the bars of tests/fuzz_parity.py; the family bar (test_moesr_gpu.MODEL_REL) is printed beside it."""

import pytest
import torch

import gaterv2_oracle as O
from sweep_common import Case as _Case
from sweep_common import _check, _input, _status_ok, acceptance, batch_of_three  # noqa: F401  (the fixture checks the status word after every test)
from test_moesr_gpu import MODEL_REL

pytestmark = pytest.mark.gpu

TWO = dict(dim=8, enc_blocks=(1, 2), dec_blocks=(2, 1), num_latent=2, scale=2, upsample='pixelshuffledirect')
SIDES2 = range(1, 10)  # 1 .. 2 P + 1


class Case(_Case):
    configs = {'two': ('gaterv2', TWO, 4, 9, 6)}
    family_bar = {'gaterv2': lambda ref: MODEL_REL * max(1.0, ref.abs().max().item())}

    def oracle(self, x, f64=True):
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            return O.gaterv2_forward(self.sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        return all((self.P - s % self.P) % self.P < s for s in (h, w))  # the reflect pad's rule; checked against the oracle below


_cases: dict = {}


def _case(name, device):
    if name not in _cases:
        _cases[name] = Case(name, device)
    return _cases[name]


def test_the_acceptance_rule_is_the_oracles():
    c = Case('two')
    for s in range(1, c.top + 1):
        for hw in (c.hw('h', s), c.hw('w', s)):
            try:
                c.oracle(torch.rand(1, c.cin, *hw))
                ran = True
            except RuntimeError:
                ran = False
            assert ran == c.accepts(*hw), hw
    assert c.legal('h') == [3, 4, 5, 6, 7, 8, 9]  # sides 1 and 2 raise


@pytest.mark.parametrize('axis', ['h', 'w'])
@pytest.mark.parametrize('s', SIDES2)
def test_two_levels_every_side(device, s, axis):
    c = _case('two', device)
    hw = c.hw(axis, s)
    if not c.accepts(*hw):
        with pytest.raises(RuntimeError, match='Padding size should be less than'):
            c.run(torch.rand(1, c.cin, *hw, device=device))
        return
    _check(c, _input(c, (1 + s % 2, c.cin, *hw), seed=100 * hw[0] + hw[1]), device, what='sweep')


def test_acceptance(device):
    acceptance(_case('two', device), device)


def test_batch_of_three(device):
    batch_of_three(_case('two', device), device, ('auto', 'bf16x3'))


def test_one_multi_tile_frame(device):
    """50 x 130 (padded to 52 x 132): more than one reduction tile on both axes at the first level, 13 x 33 = 429 latent tokens (four token
    chunks, the last one ragged)."""
    c = _case('two', device)
    _check(c, _input(c, (1, c.cin, 50, 130), seed=17), device, what='multi-tile')
