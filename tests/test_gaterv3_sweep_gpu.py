"""Whole-model GPU sweep of GateRV3 over input sizes, on tests/sweep_common.py, against the float64 oracle (tests/gaterv3_oracle.py):
every side from 1 to 2 P + 1 on either axis for a two-level model (P = 4), the legal sides around 9, 16 and 17 for a four-level one
(P = 16), acceptance exactly where the oracle raises, a batch of three with different statistics per image (sca's mean is per image), every
head, the plan cache across sizes, the precision switch, one multi-tile frame (more than one reduction tile and more than one token chunk),
and dtypes and layouts.  Every case runs twice, the second run bit-equal.  Tolerance (asserted): sweep_common.FUZZ_BAR, the bars of
tests/fuzz_parity.py; the family bar (test_moesr_gpu.MODEL_REL) is printed beside it."""

import pytest
import torch

import gaterv3_oracle as O
from sweep_common import Case as _Case
from sweep_common import _check, _input, _status_ok, acceptance, batch_of_three, dtypes_and_layouts  # noqa: F401  (the fixture checks the status word after every test)
from test_moesr_gpu import MODEL_REL

pytestmark = pytest.mark.gpu

TWO = dict(dim=8, enc_blocks=(1, 2), dec_blocks=(2, 1), num_latent=2, span_blocks=1, scale=2, upsample='pixelshuffledirect')
FOUR = dict(dim=8, enc_blocks=(1, 1, 1, 1), dec_blocks=(1, 1, 1, 1), num_latent=1, span_blocks=1, attention=True)
HEADS = {
    'psd x3': dict(TWO, scale=3), 'ps x4': dict(TWO, scale=4, upsample='pixelshuffle', upsample_mid_dim=16), 'nc x2': dict(TWO, upsample='nearest+conv'),
    'nc x3': dict(TWO, scale=3, upsample='nearest+conv'), 'dys x2 front k3': dict(TWO, upsample='dysample', upsample_mid_dim=16, end_kernel=3),
    'dys x3 k1': dict(TWO, scale=3, upsample='dysample', upsample_mid_dim=8, end_kernel=1), 'x1': dict(TWO, scale=1),
}  # fmt: skip
SIDES2 = range(1, 10)  # 1 .. 2 P + 1
SIDES4 = (9, 10, 15, 16, 17, 18)


class Case(_Case):
    configs = dict({'two': ('gaterv3', TWO, 4, 9, 6), 'four': ('gaterv3', FOUR, 16, 18, 16)}, **{k: ('gaterv3', kw, 4, 9, 6) for k, kw in HEADS.items()})
    family_bar = {'gaterv3': lambda ref: MODEL_REL * max(1.0, ref.abs().max().item())}

    def oracle(self, x, f64=True):
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            return O.gaterv3_forward(self.sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        return all((self.P - s % self.P) % self.P < s for s in (h, w))  # the reflect pad's rule; checked against the oracle below


_cases: dict = {}


def _case(name, device):
    if name not in _cases:
        _cases[name] = Case(name, device)
    return _cases[name]


def test_the_acceptance_rule_is_the_oracles():
    for name in ('two', 'four'):
        c = Case(name)
        for s in range(1, c.top + 1):
            for hw in (c.hw('h', s), c.hw('w', s)):
                try:
                    c.oracle(torch.rand(1, c.cin, *hw))
                    ran = True
                except RuntimeError:
                    ran = False
                assert ran == c.accepts(*hw), (name, hw)
    two, four = Case('two'), Case('four')
    assert two.legal('h') == [3, 4, 5, 6, 7, 8, 9] and four.legal('w') == list(range(9, 19))  # sides 1 and 2 raise; so does 8 with four levels


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


@pytest.mark.parametrize('axis', ['h', 'w'])
@pytest.mark.parametrize('s', SIDES4)
def test_four_levels_around_9_16_17(device, s, axis):
    c = _case('four', device)
    hw = c.hw(axis, s)
    _check(c, _input(c, (1, c.cin, *hw), seed=100 * hw[0] + hw[1]), device, what='sweep')


@pytest.mark.parametrize('name', ['two', 'four'])
def test_acceptance(device, name):
    acceptance(_case(name, device), device)


def test_batch_of_three_and_the_precision_switch(device):
    batch_of_three(_case('two', device), device, ('auto', 'bf16x3'))
    c = _case('two', device)
    x = _input(c, (1, c.cin, 7, 6), seed=9)
    y, _ = _check(c, x, device, what='before the switch')
    for precision in ('fp16', 'bf16'):
        c.m.precision = precision
        z = c.m(x.to(device)).cpu().double()
        print(f'MEASURE gaterv3 [two] {precision}: max-abs against bf16x3 {(z - y).abs().max().item():.3e}')
        assert torch.isfinite(z).all() and not torch.equal(z, y)
    y2, _ = _check(c, x, device, what='after the switch')
    assert torch.equal(y2, y)  # back to the cached plan of the first mode


@pytest.mark.parametrize('name', sorted(HEADS))
def test_every_head(device, name):
    c = _case(name, device)
    _check(c, _input(c, (2, c.cin, 5, 7), seed=31), device, what='heads')


def test_plan_cache_across_sizes(device):
    c = _case('two', device)
    xs = [_input(c, (1, c.cin, h, w), seed=3 + h) for h, w in ((5, 6), (8, 9), (3, 3), (5, 6))]
    first = [_check(c, x, device, what='plan cache')[0] for x in xs]
    assert torch.equal(first[0], first[3])
    for x, y0 in zip(xs, first):
        assert torch.equal(c.m(x.to(device)).cpu().double(), y0)


def test_one_multi_tile_frame(device):
    """200 x 300 (padded to 208 x 304): more than one reduction tile on both axes at every level of the encoder, 13 x 19 = 247 latent tokens
    (two token chunks)."""
    c = _case('four', device)
    _check(c, _input(c, (1, c.cin, 200, 300), seed=17), device, what='multi-tile')


def test_dtypes_and_layouts(device):
    dtypes_and_layouts(_case('two', device), device, ('auto',), 'auto')
