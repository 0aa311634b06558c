"""End-to-end GPU parity of FIGSR against the reference's vectors (tools/gen_golden_figsr.py) and against the float64 oracle
(tests/figsr_oracle.py) over a sweep of sizes.

Tolerance: max-abs <= 2e-4 * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3', GFISRv2's bar (the FourierUnit and the
convolution arithmetic are the same).  Every case prints a MEASURE line; profiles/figsr_sweep_measure.txt keeps them.
figsr_x4_psd_d48_b24_9x11 is the depth check: the default 24 blocks.  The sweep runs a dim 32, two-block x2 model through
tests/sweep_common.py (its ``Case`` and ``_check``: every size twice, the second run bit-equal): every H in 6..11 beside W = 24 and
every W in 22..27 beside H = 8 -- the padded sizes 14..20 and 30..36 straddle the 16 and 32 tile edges.  Then batch 2 against two single
runs, fp16 / bf16 tensors in and out at the 1e-2 bar of test_cugan_gpu.test_half_and_bfloat16_io, the plan cache, the refusals (before
any launch) and tiling.
"""

import warnings

import pytest
import torch

import figsr_oracle as O
import resselt_amd
import sweep_common as S
from helpers import golden_names, load_golden
from resselt_amd.archs.figsr.arch import FIGSR
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.utils import synth
from sweep_common import _status_ok  # noqa: F401  (autouse: rsa_check_status() == 0 after every test)

pytestmark = pytest.mark.gpu

MODEL_REL = 2e-4  # whole models: max-abs <= MODEL_REL * max(1, |y|max) (tests/test_gfisrv2_gpu.py)
NAMES = [n for n in golden_names('figsr_') if n != 'figsr_probe']
SWEEP = [(h, 24) for h in range(6, 12)] + [(8, w) for w in range(22, 28)]


def _sd(meta):
    return synth.figsr_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures():
    assert len(NAMES) == 11


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert isinstance(m, FIGSR) and m.resolved_precision() == 'bf16x3'
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e})')
    assert err <= MODEL_REL * max(1.0, arr['y'].abs().max().item()), f'{name} {precision}: max-abs {err:.3e}'
    y2 = m(arr['x'].to(device))  # second call: the cached plan
    assert torch.equal(y2, y)


@pytest.mark.parametrize('name', NAMES)
def test_fp16_mode_runs(device, name):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m.precision = 'fp16'
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape and torch.isfinite(y).all()
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} fp16: max-abs {err:.3e}')
    assert err <= 3e-2 * max(1.0, arr['y'].abs().max().item())  # the one-product benchmark mode at the bar tests/test_gfisrv2_gpu.py gives it


class Case(S.Case):
    """The sweep's configuration, on tests/sweep_common.py's ``Case``; the oracle is this family's own (helpers.oracle_forward does not know it)."""

    configs = {'figsr_x2': ('figsr', dict(dim=32, n_blocks=2, scale=2), 2, (11, 27), 24)}
    family_bar = {'figsr': lambda ref: MODEL_REL * max(1.0, ref.abs().max().item())}

    def oracle(self, x, f64=True):
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            return O.figsr_forward(self.sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        return h >= 6 and w >= 6


@pytest.fixture(scope='module')
def sweep_case(device):
    return Case('figsr_x2', device)


@pytest.mark.parametrize('hw', SWEEP, ids=[f'{h}x{w}' for h, w in SWEEP])
def test_size_sweep_against_the_float64_oracle(device, sweep_case, hw):
    c = sweep_case
    x = S._input(c, (1, 3, *hw), seed=100 * hw[0] + hw[1])
    got, ref = S._check(c, x, device, what='size sweep')
    err, bar = (got - ref).abs().max().item(), c.family_bar['figsr'](ref)
    assert err <= bar, f'{hw}: max-abs {err:.3e} > {bar:.3e}; {S._where(got, ref, c.P, hw)}'


def test_batch_of_two_against_two_single_runs(device, sweep_case):
    m = sweep_case.m
    m.precision = 'auto'
    x = S._images((2, 3, 7, 9), seed=5).to(device)
    both = m(x).cpu()
    singles = torch.cat([m(x[i : i + 1].contiguous()).cpu() for i in range(2)])
    assert both.shape == (2, 3, 14, 18) and torch.equal(both, singles)


@pytest.mark.parametrize('dt', [torch.float16, torch.bfloat16], ids=['float16', 'bfloat16'])
def test_half_and_bfloat16_io(device, sweep_case, dt):
    c = sweep_case
    c.m.precision = 'auto'
    x = S._input(c, (2, 3, 9, 8), seed=41, dt=dt).to(dt)
    ref = c.oracle(x)
    y = c.m(x.to(device))
    torch.cuda.synchronize()
    assert y.dtype == dt and y.shape == ref.shape
    err = (y.float().cpu().double() - ref).abs().max().item()
    print(f'MEASURE figsr [figsr_x2] {str(dt)[6:]} tensors in and out: max-abs {err:.3e} (bar {1e-2 * max(1.0, ref.abs().max().item()):.1e})')
    assert err <= 1e-2 * max(1.0, ref.abs().max().item())


def test_plan_cache_round_trip(device, sweep_case):
    """Two sizes alternating through one model: each size keeps its plan (DFT tables included), and a plan evicted and rebuilt gives the
    same bits."""
    m = sweep_case.m
    m.precision = 'auto'
    xs = [synth.synth_input((1, 3, 7, 10), 77).to(device), synth.synth_input((1, 3, 10, 7), 78).to(device)]
    first = [m(x).clone() for x in xs]
    held = len(m._plans)
    for x, y0 in zip(xs, first):
        assert torch.equal(m(x), y0)
    assert len(m._plans) == held  # nothing was rebuilt
    m.invalidate()
    assert len(m._plans) == 0
    for x, y0 in zip(xs, first):
        assert torch.equal(m(x), y0)


def test_launch_count(device):
    """Per block nine launch steps, eleven kernels (a transform is two): rsa_rmsnorm, fc1, forward DFT, rsa_gfisr_spectral, fdc, inverse DFT,
    rsa_plk_conv, rsa_figsr_mix, fc2; around them in_to_dim, the 3x3 behind the second half, cat_to_dim, the head's one convolution and
    rsa_figsr_output."""
    meta, arr = load_golden('figsr_x2_psd_d32_b2_n2_6x8')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_gfisr_dft') == 4 and calls.count('rsa_gfisr_spectral') == 2 and calls.count('rsa_plk_conv') == 2 and calls.count('rsa_figsr_mix') == 2
    assert 'rsa_gfisr_gate' not in calls
    assert m.launches_per_forward() == 11 * 2 + 5  # (the plan does not count the conversion of the caller's input into planes)


def test_every_refusal_raises_before_any_launch(device):
    lib = L.load()
    meta, _ = load_golden('figsr_probe')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    for p in meta['probe']:
        if p['raises'] is not None:
            with pytest.raises(RuntimeError, match='Padding size should be less'):
                m(torch.rand(1, 3, *p['size'], device=device))
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m(torch.rand(1, 1, 9, 9, device=device))
    torch.cuda.synchronize()
    assert lib.rsa_check_status() == 0 and m.launches_per_forward() is None  # no plan was ever built
    for kw, text in ((dict(in_nc=1, out_nc=1), '3 input and 3 output'), (dict(gc=4, square_kernel_size=7, band_kernel_size=11), 'gc must be 8 or 16'),
                     (dict(band_kernel_size=33), 'band kernel size'), (dict(n_blocks=4, halves=(1, 3)), 'halves must be the')):  # fmt: skip
        with pytest.raises(NotImplementedError, match=text):
            resselt_amd.load_from_state_dict(dict(synth.figsr_state_dict(**dict(dict(dim=32, n_blocks=2, scale=2), **kw))))
    y = m(torch.rand(1, 3, 6, 6, device=device))  # the module still works
    assert y.shape == (1, 3, 12, 12) and torch.isfinite(y).all()


def test_upscale_with_one_tile_equals_the_plain_forward(device):
    meta, arr = load_golden('figsr_x2_dys_d32_m16_b2_6x6')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    img = (torch.rand(9, 11, 3, generator=torch.Generator().manual_seed(3)) * 255).to(torch.uint8).to(device)
    with warnings.catch_warnings():
        warnings.simplefilter('error')  # one tile: nothing to warn about
        out = resselt_amd.upscale(m, img, dtype=torch.float32)
    plain = ops.nchw_to_image_u8(m(ops.image_u8_to_nchw(img, torch.float32)))[0]
    assert out.shape == (18, 22, 3) and out.dtype == torch.uint8 and torch.equal(out, plain)
    assert torch.equal(resselt_amd.upscale(m, img, tile=(16, 16), dtype=torch.float32), out)  # the image fits one tile
    with pytest.warns(RuntimeWarning, match='normalises over the whole image'):  # the FourierUnit spans the tensor it is given
        tiled = resselt_amd.upscale(m, img, tile=(6, 6), halo=3, dtype=torch.float32)  # (every tile with its halo has at least 6 rows and columns)
    assert tiled.shape == out.shape
