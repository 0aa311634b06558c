"""``rsa_tile_blend_accumulate`` (csrc/tile_blend.hip) alone, against f64 computed from the exact source values.

Every case (source format x channels x batch) walks all 16 subsets of the four ramps at the ramp widths 2 (the minimum: blend * scale = 1),
6 and 24, over window widths that are ragged against the 4-pixel vectors and the 1024-pixel workgroup rows (1 + ramp, 7, 33, 65, 257) and
heights from 3 to 40, at non-zero source and accumulator offsets, with accumulator rows on and off 16-byte boundaries.

The accumulator is pre-filled with NaN where the rule says STORE (no earlier contributor: neither the top nor the left ramp), with known
random values where it says ACCUMULATE, and with a sentinel outside the window, which must come back bit for bit.

Tolerance 2^-21 * max(1, |y|max, |acc|max): the ramp, the product of the two ramps, the multiply and the add are four f32 roundings
(2.4e-7 relative), with a margin of two; the falling ramp's ``1 - u`` and the ``code / 255`` of an 8-bit source are roundings of the same size
and fit the margin, and the kernel fuses the multiply-add."""

import itertools

import pytest
import torch

import tile_blend_reference as R
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops

pytestmark = pytest.mark.gpu

TOL = 2.0**-21
RAMP_WIDTHS = (2, 6, 24)
WIDTHS = (7, 33, 65, 257)
HEIGHTS = (3, 5, 8, 13, 26, 40)
ACC_SIZES = ((96, 320), (95, 317), (96, 318))  # rows of the second and third start off 16-byte boundaries; 95 * 317 is odd (planes too)


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _combos():
    """(ramps, window, src_offset, acc_offset, acc_size) of the 48 launches of one case."""
    out = []
    for i, (subset, r) in enumerate(itertools.product(itertools.product((0, 1), repeat=4), RAMP_WIDTHS)):
        top, bottom, left, right = (r * bit for bit in subset)
        widths = (1 + r,) + tuple(w for w in WIDTHS if w >= r)
        win_w = widths[(i * 3 + i // 5) % len(widths)]
        win_h = HEIGHTS[(i * 5 + i // 7) % len(HEIGHTS)]
        if win_h < max(top, bottom):
            win_h = r + 1
        out.append(((top, bottom, left, right), (win_h, win_w), ((3, 1)[i % 2], (5, 8, 2)[i % 3]), ((2, 7)[i % 2], (4, 9, 16, 3)[i % 4]), ACC_SIZES[(i // 2) % 3]))
    return out


def test_the_combinations_cover_what_they_claim():
    combos = _combos()
    assert [k for k, _ in L.INTERNAL['rsa_tile_blend_accumulate'][1]][-5:] == ['ramp_top', 'ramp_bottom', 'ramp_left', 'ramp_right', 'stream']  # the order of `ramps`
    assert len(combos) == 48 and {c[0] for c in combos} >= {tuple(r * b for b in s) for s in itertools.product((0, 1), repeat=4) for r in RAMP_WIDTHS}
    assert {c[1][1] for c in combos} == {3, 7, 25, 33, 65, 257} and min(c[1][0] for c in combos) == 3 and max(c[1][0] for c in combos) == 40
    assert all(ay + wh <= ah and ax + ww <= aw for _, (wh, ww), _, (ay, ax), (ah, aw) in combos)


def _source(fmt, n, c, h, w, g):
    """(tensor as the kernel reads it, its exact values as f64 [N, C, h, w])."""
    if fmt == 'u8':
        img = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)
        return img, R.image_as_f64(img)
    y = ((torch.rand((n, c, h, w), generator=g) * 4 - 2).to({'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[fmt]))
    return y, y.double()


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('fmt', ['f32', 'f16', 'bf16', 'u8'])
def test_accumulate_against_f64(device, fmt, c, n):
    g = torch.Generator().manual_seed(1000 + 10 * c + n)
    worst = 0.0
    for ramps, (wh, ww), (sy, sx), (ay, ax), (ah, aw) in _combos():
        top, bottom, left, right = ramps
        y, y64 = _source(fmt, n, c, sy + wh + 2, sx + ww + 3, g)
        sentinel = torch.rand((n, c, ah, aw), generator=g) * 6 - 3
        prior = torch.rand((n, c, wh, ww), generator=g) * 6 - 3
        adds = torch.zeros(wh, ww, dtype=torch.bool)
        adds[:top] = True
        adds[:, :left] = True
        before = sentinel.clone()
        before[:, :, ay : ay + wh, ax : ax + ww] = torch.where(adds, prior, torch.full_like(prior, float('nan')))
        want = sentinel.double()
        wgt = R.ramp_weights(wh, top, bottom)[:, None] * R.ramp_weights(ww, left, right)[None, :]
        want[:, :, ay : ay + wh, ax : ax + ww] = torch.where(adds, prior.double(), torch.zeros((), dtype=torch.float64)) + wgt * y64[:, :, sy : sy + wh, sx : sx + ww]

        runs = []
        for _ in range(2):
            acc = before.clone().to(device)
            ops.tile_blend_accumulate(acc, y.to(device), (wh, ww), (sy, sx), (ay, ax), ramps)
            runs.append(acc.cpu())
        got = runs[0]
        what = f'{fmt} C={c} N={n} ramps={ramps} window={wh}x{ww} src+({sy},{sx}) acc+({ay},{ax}) of {ah}x{aw}'
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), f'{what}: two runs differ'
        outside = torch.ones(ah, aw, dtype=torch.bool)
        outside[ay : ay + wh, ax : ax + ww] = False
        assert torch.equal(got[..., outside].view(torch.int32), sentinel[..., outside].view(torch.int32)), f'{what}: wrote outside the window'
        inside = got[:, :, ay : ay + wh, ax : ax + ww]
        assert bool(torch.isfinite(inside).all()), f'{what}: a stored pixel kept its NaN'
        err = (inside.double() - want[:, :, ay : ay + wh, ax : ax + ww]).abs().max().item()
        bound = TOL * max(1.0, y64.abs().max().item(), prior.abs().max().item())
        worst = max(worst, err / bound)
        assert err <= bound, f'{what}: max-abs {err:.3e} > {bound:.3e}'
    print(f'MEASURE tile_blend {fmt} C={c} N={n}: worst error {worst:.3f} of the bound over 48 launches')
