"""What makes the bounds of tests/norm_reference.py worth holding a kernel to, checked without a GPU for every case the GPU tests run:

1. the correct float32 emulations (both forms of the normalise step, GELU(LayerNorm), RMSNorm) stay inside the bound at every element, also
   after rounding to each plane format with that format's term added;
2. the bound of every case is at most 2^-6 of the case's max |ref|, and E <= E_MAX, which the second-order factor assumes;
3. each deliberately wrong emulation leaves the bound in the case that is there to catch it: the one-pass variance at the worst-conditioned
   case, the padded-count divisor at every swept C that is not a multiple of 4, the missing eps at the constant pixel.
"""

import pytest
import torch

import norm_reference as R

IDS = [c.name for c in R.ALL_CASES]


def _emulate(case, d, form='centred', wrong=None):
    a = (d['x'], d['gamma'], d['beta'], d['eps'])
    if case.op == 'ln':
        return R.emulate_layernorm(*a, form=form, wrong=wrong)
    return R.emulate_layernorm_gelu(*a) if case.op == 'gelu' else R.emulate_rmsnorm(*a)


def _outside(got, ref, bound):
    """Elements that are not inside the bound (a NaN is outside)."""
    return ~((got.double() - ref).abs() <= bound)


@pytest.mark.parametrize('case', R.ALL_CASES, ids=IDS)
def test_correct_emulations_inside_a_useful_bound(case):
    d = R.make_case(case)
    for form in ('centred', 'nm') if case.op == 'ln' else ('centred',):
        ref, bound = R.reference(case, d, form)
        got = _emulate(case, d, form)
        err = (got.double() - ref).abs()
        print(f'MEASURE emulation {case.name} {form}: worst error / bound {float((err / bound).max()):.3f}, bound max {float(bound.max()):.3e}, '
              f'|ref|max {float(ref.abs().max()):.3f}, ratio {d["ratio"]:g}')  # fmt: skip
        assert not _outside(got, ref, bound).any()  # condition 1
        assert float(bound.max()) <= R.USEFUL * float(ref.abs().max())  # condition 2
    assert R.case_e(case, d) <= R.E_MAX
    assert R.useful(case, d)


@pytest.mark.parametrize('case', R.FORMS + R.GELU[4:6] + R.RMS[4:6], ids=lambda c: c.name)
def test_emulations_through_the_plane_formats(case):
    d = R.make_case(case)
    ref, bound = R.reference(case, d)
    got = _emulate(case, d)
    for fmt in (R.PF_BF16, R.PF_F16, None):
        for with_lo in (True, False):
            held = R.round_to_planes(got, fmt, with_lo)
            assert not _outside(held, ref, bound + R.plane_term(ref, fmt, with_lo)).any(), (fmt, with_lo)


def test_max_ratio_is_the_largest_useful_power_of_two():
    for case in R.CONDITIONING:
        if case.ratio != R.MAX:
            continue
        r = R.max_ratio(case)
        assert r >= 64 and R.useful(case, R._build(case, r)) and not R.useful(case, R._build(case, 2 * r)), case.name
        assert r > 30.0  # three distinct levels


def test_one_pass_variance_is_caught_at_the_worst_conditioned_case():
    d = R.make_case(R.WORST)
    assert R.WORST.C == max(R.COND_C) and R.WORST.eps == min(R.COND_EPS) and d['ratio'] == R.max_ratio(R.WORST)
    for form in ('centred', 'nm'):
        ref, bound = R.reference(R.WORST, d, form)
        assert _outside(_emulate(R.WORST, d, form, 'one_pass'), ref, bound).any()
    # and it is the conditioning that catches it: at offset / sigma = 1 the one-pass variance is as good as the centred one
    easy = next(c for c in R.CONDITIONING if c.C == 400 and c.eps == 1e-6 and c.ratio == 1.0)
    de = R.make_case(easy)
    ref, bound = R.reference(easy, de)
    assert not _outside(_emulate(easy, de, 'centred', 'one_pass'), ref, bound).any()


@pytest.mark.parametrize('case', R.SWEEP, ids=lambda c: c.name)
def test_padded_count_is_caught_where_c_is_no_multiple_of_four(case):
    d = R.make_case(case)
    ref, bound = R.reference(case, d)
    bad = _outside(_emulate(case, d, 'centred', 'padded_count'), ref, bound)
    if case.C == 1:  # one channel: d_c = 0 whatever the mean's divisor... but not in f32: x - x / 4 is far from 0
        assert bad.any()
    elif case.C % 4:
        assert bad.any()
    else:
        assert not bad.any()  # the same arithmetic


@pytest.mark.parametrize('case', R.CONDITIONING, ids=lambda c: c.name)
def test_missing_eps_is_caught_at_the_constant_pixel(case):
    d = R.make_case(case)
    n, y, x = d['const_tok']
    ref, bound = R.reference(case, d)
    assert bool((ref[n, :, y, x] - d['beta'].double()).abs().max() == 0)  # f64: a constant pixel comes out as beta
    got = _emulate(case, d, 'centred', 'no_eps')
    assert _outside(got[n, :, y, x], ref[n, :, y, x], bound[n, :, y, x]).any()
    zn, zy, zx = d['zero_tok']
    assert bool((ref[zn, :, zy, zx] == d['beta'].double()).all())


def test_bracket_cases_share_their_statistics():
    """The three embeddings of the same 180 channels: mean and variance of every token agree up to the f32 rounding of the fill values."""
    base = R.make_case(R.BRACKETS[0])
    m0, d0, _ = R.ln_stats(base['x'], 0.0)
    v0 = (d0 * d0).mean(1, keepdim=True)
    for case in R.BRACKETS[1:]:
        d = R.make_case(case)
        assert torch.equal(d['x'][:, :180], base['x']) and torch.equal(d['gamma'][:180], base['gamma'])
        assert not d['gamma'][180:].any() and not d['beta'][180:].any()
        m, dd, _ = R.ln_stats(d['x'], 0.0)
        v = (dd * dd).mean(1, keepdim=True)
        scale = m0.abs() + v0.sqrt()
        assert bool(((m - m0).abs() <= 2 * R.U * scale).all()) and bool(((v - v0).abs() <= 8 * R.U * scale * v0.sqrt()).all())
