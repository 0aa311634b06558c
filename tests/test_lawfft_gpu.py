"""End-to-end GPU parity of LAWFFT against the reference's vectors (tools/gen_golden_lawfft.py) and against the float64 oracle
(tests/lawfft_oracle.py) over a sweep of sizes.

Tolerance: max-abs <= 2e-4 * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3', the project's model bar; a fixture whose
own f32-f64 deviation exceeded a quarter of that bar would take 4 x that deviation instead (``_bar`` says so; no fixture does, and
``test_fixtures`` holds them to that).  Every case prints a MEASURE line; profiles/lawfft_sweep_measure.txt keeps them.
lawfft_x4_psd_d60_r4_m6_9x11 is the depth check: the default 4 x 6 blocks.  The sweep runs a dim 32 (local 8), one-group, two-block x2 model
through tests/sweep_common.py (its ``Case`` and ``_check``: every size twice, the second run bit-equal): every H in 6..11 beside W = 24 and
every W in 22..27 beside H = 8 -- both sides of the multiples of 8.  Then batch 2 against two single runs, fp16 / bf16 tensors in and out
at the 1e-2 bar of test_cugan_gpu.test_half_and_bfloat16_io, the plan cache, the refusals (before any launch) and tiling.
"""

import warnings

import pytest
import torch

import lawfft_oracle as O
import resselt_amd
import sweep_common as S
from helpers import golden_names, load_golden
from resselt_amd.archs.lawfft.arch import LAWFFT
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.utils import synth
from sweep_common import _status_ok  # noqa: F401  (autouse: rsa_check_status() == 0 after every test)

pytestmark = pytest.mark.gpu

MODEL_REL = 2e-4  # whole models: max-abs <= MODEL_REL * max(1, |y|max) (tests/test_gfisrv2_gpu.py)
NAMES = [n for n in golden_names('lawfft_') if n != 'lawfft_probe']
SWEEP = [(h, 24) for h in range(6, 12)] + [(8, w) for w in range(22, 28)]


def _sd(meta):
    return synth.lawfft_state_dict(seed=meta['seed'], **meta['synth'])


def _bar(meta, y):
    """The model bar; 4 x the fixture's own f32-f64 deviation where that deviation exceeds a quarter of it."""
    bar = MODEL_REL * max(1.0, y.abs().max().item())
    return 4 * meta['f64_dev'] if meta['f64_dev'] > bar / 4 else bar


def test_fixtures():
    assert len(NAMES) == 11
    for n in NAMES:
        meta, arr = load_golden(n)
        assert meta['f64_dev'] <= MODEL_REL * max(1.0, arr['y'].abs().max().item()) / 4, n  # every fixture takes the model bar itself


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert isinstance(m, LAWFFT) and m.resolved_precision() == 'bf16x3'
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f}; the reference\'s own f32-f64 {meta["f64_dev"]:.2e}; bar {_bar(meta, arr["y"]):.2e})')
    assert err <= _bar(meta, arr['y']), f'{name} {precision}: max-abs {err:.3e}'
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

    configs = {'lawfft_x2': ('lawfft', dict(dim=32, local=8, n_rblock=1, n_mblock=2, scale=2), 8, (11, 27), 24)}
    family_bar = {'lawfft': lambda ref: MODEL_REL * max(1.0, ref.abs().max().item())}

    def oracle(self, x, f64=True):
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            return O.lawfft_forward(self.sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        return h >= 5 and w >= 5


@pytest.fixture(scope='module')
def sweep_case(device):
    return Case('lawfft_x2', device)


@pytest.mark.parametrize('hw', SWEEP, ids=[f'{h}x{w}' for h, w in SWEEP])
def test_size_sweep_against_the_float64_oracle(device, sweep_case, hw):
    c = sweep_case
    x = S._input(c, (1, 3, *hw), seed=100 * hw[0] + hw[1])
    got, ref = S._check(c, x, device, what='size sweep')
    err, bar = (got - ref).abs().max().item(), c.family_bar['lawfft'](ref)
    assert err <= bar, f'{hw}: max-abs {err:.3e} > {bar:.3e}; {S._where(got, ref, c.P, hw)}'


def test_batch_of_two_against_two_single_runs(device, sweep_case):
    m = sweep_case.m
    m.precision = 'auto'
    x = S._images((2, 3, 7, 9), seed=5).to(device)
    both = m(x).cpu()
    singles = torch.cat([m(x[i : i + 1].contiguous()).cpu() for i in range(2)])
    assert both.shape == (2, 3, 14, 18) and torch.equal(both, singles)
    assert not torch.equal(both[0], both[1])


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
    print(f'MEASURE lawfft [lawfft_x2] {str(dt)[6:]} tensors in and out: max-abs {err:.3e} (bar {1e-2 * max(1.0, ref.abs().max().item()):.1e})')
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
    """Per MetaBlock 13 launch steps and 15 kernels windowed (a kernel generator is two), 17 steps and 22 kernels whole-image (a transform
    is two); around them in_to_dim, a group's DynamicLocal (3 kernels) and the head's one convolution."""
    meta, arr = load_golden('lawfft_x2_psd_d32_r1_m2_n2_8x16')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_lawfft_wincorr') == 1 and calls.count('rsa_gfisr_dft') == 3 and calls.count('rsa_lawfft_spec_mul') == 1 and calls.count('rsa_lawfft_norm_mul') == 1
    assert calls.count('rsa_lawfft_kernel_gen') == 5 and calls.count('rsa_lawfft_dyn_dwconv') == 5 and calls.count('rsa_eimn_sal') == 2
    assert m.launches_per_forward() == 22 + 15 + 1 + 3 + 1  # (the plan does not count the conversion of the caller's input into planes)


def test_every_refusal_raises_before_any_launch(device):
    lib = L.load()
    meta, _ = load_golden('lawfft_probe')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    for p in meta['probe']:
        if p['raises'] is not None:
            with pytest.raises(RuntimeError, match='Padding size should be less'):
                m(torch.rand(1, 3, *p['size'], device=device))
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m(torch.rand(1, 1, 9, 9, device=device))
    torch.cuda.synchronize()
    assert lib.rsa_check_status() == 0 and m.launches_per_forward() is None  # no plan was ever built
    base = dict(dim=32, local=8, n_rblock=1, n_mblock=2, scale=2)
    for kw, text in ((dict(window_size=4), 'window_size 4 is not built'), (dict(n_mblock=1), 'at least two MetaBlocks'), (dict(to_hidden_rows=71), '3 x the FSAS width')):
        with pytest.raises(NotImplementedError, match=text):
            resselt_amd.load_from_state_dict(dict(synth.lawfft_state_dict(**dict(base, **kw))))
    both = synth.lawfft_state_dict(**base)
    both['in_to_dim.1.weight'] = torch.zeros(32, 12, 3, 3)
    with pytest.raises(NotImplementedError, match='unshuffle_mod'):
        resselt_amd.load_from_state_dict(dict(both))
    y = m(torch.rand(1, 3, 5, 5, device=device))  # the module still works, at the smallest legal size
    assert y.shape == (1, 3, 10, 10) and torch.isfinite(y).all()


def test_probe_sizes_match_the_reference(device):
    meta, arr = load_golden('lawfft_probe')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    for p in meta['probe']:
        if p['raises'] is None:
            h, w = p['size']
            y = m(arr[f'x_{h}x{w}'].to(device)).cpu()
            ref = arr[f'y_{h}x{w}']
            err = (y - ref).abs().max().item()
            print(f'MEASURE lawfft_probe {h}x{w}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
            assert err <= MODEL_REL * max(1.0, ref.abs().max().item())


def test_the_float_split_checkpoint_runs(device):
    """The (dim, local) pair the reference's own module rejects: the engine reads the widths from the shapes, and runs it."""
    meta, _ = load_golden('lawfft_probe')
    fs = meta['float_split']
    sd = synth.lawfft_state_dict(seed=meta['seed'], **fs['synth'])
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    x = synth.synth_input((1, 3, 9, 10), 3)
    y = m(x.to(device)).cpu()
    with torch.no_grad():
        ref = O.lawfft_forward(sd, x.double())
    err = (y.double() - ref).abs().max().item()
    print(f'MEASURE lawfft float-split dim {fs["synth"]["dim"]} local {fs["synth"]["local"]}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= MODEL_REL * max(1.0, ref.abs().max().item())


def test_upscale_with_one_tile_equals_the_plain_forward(device):
    meta, arr = load_golden('lawfft_x2_dys_d32_m16_r2_m2_6x9')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    img = (torch.rand(9, 11, 3, generator=torch.Generator().manual_seed(3)) * 255).to(torch.uint8).to(device)
    with warnings.catch_warnings():
        warnings.simplefilter('error')  # one tile: nothing to warn about
        out = resselt_amd.upscale(m, img, dtype=torch.float32)
    plain = ops.nchw_to_image_u8(m(ops.image_u8_to_nchw(img, torch.float32)))[0]
    assert out.shape == (18, 22, 3) and out.dtype == torch.uint8 and torch.equal(out, plain)
    assert torch.equal(resselt_amd.upscale(m, img, tile=(16, 16), dtype=torch.float32), out)  # the image fits one tile
    with pytest.warns(RuntimeWarning, match='normalises over the whole image'):  # the pooling and the whole-image correlation span the tensor given
        tiled = resselt_amd.upscale(m, img, tile=(6, 6), halo=3, dtype=torch.float32)  # (every tile with its halo has at least 5 rows and columns)
    assert tiled.shape == out.shape
