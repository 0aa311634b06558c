"""End-to-end GPU parity of ATD against the reference's vectors (tools/gen_golden_atd.py) and the CPU oracle (tests/atd_oracle.py).

1. Forced: every fixture with the reference's recorded permutations forced (``atd_force``): max-abs <= 3e-4 * max(1, max|y|) in 'auto'
   (= 'bf16x3') and 'bf16x3', 3e-2 in 'bf16', 2e-3 with fp16 tensor I/O; the second run of the cached plan is bit-identical.
2. Free-running on the guarded fixtures (smallest top-two margin >= TAU): the recorded ids equal those of the reference's stable run, the
   recorded permutation is the stable sort of the ids, the output is within tolerance of ``y_stable``.
3. Larger inputs without fixture: the engine runs free with recording on; the oracle then runs with the engine's permutations forced and
   computes its own ids along that trajectory.  The output is within tolerance of that run, the engine's permutation is exactly the stable
   sort of its ids, every differing id decision has an oracle top-two margin below TAU, and at most 0.2 % of the decisions differ.
4. ``upscale()`` on uint8; inputs below half a window (which one flip cannot pad to a window, and the reference fails on) raise before
   any launch; from half a window on they run (test_newer_archs_sweep_gpu.py compares the refusals with the oracle's side by side).

The id conditions of 2 and 3 hold in three bf16 products.  In the one-product 'bf16' mode the similarity path is f32 as well, but the
residual stream it reads is computed with 8-bit operands (the 3e-2 tolerance), so decisions with margins far above TAU legitimately move:
there the output is compared on the engine's own trajectory (3) and the permutation must still be the stable sort of the engine's ids.
"""

import pytest
import torch

import atd_oracle as O
import resselt_amd
from atd_trajectory import run_on_engine_trajectory
from helpers import golden_names, load_golden
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NAMES = golden_names('atd_')
GUARDED = [n for n in NAMES if load_golden(n)[0]['guarded']]


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _tol(ref, rel=3e-4):
    return rel * max(1.0, ref.abs().max().item())


def _case(name):
    meta, arr = load_golden(name)
    sd = synth.atd_state_dict(seed=meta['seed'], **meta['synth'])
    return meta, arr, sd


def _run(m, x, device, crop):
    y = m(x.to(device))
    torch.cuda.synchronize()
    return (y[:, :, : crop[1], : crop[3]] if crop else y).float().cpu()


def _forced(meta, arr, device):
    return [arr[f'perm_{li}'].to(device) for li in range(meta['layers'])]


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_forced_matches_reference_vectors(device, name, precision):
    meta, arr, sd = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    assert m.resolved_precision() == 'bf16x3'
    m.atd_force = _forced(meta, arr, device)
    y = _run(m, arr['x'], device, meta.get('crop'))
    ref = arr['y']
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    print(f'{name} {precision}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert err <= _tol(ref), f'{name} {precision}: max-abs {err:.3e}'
    assert torch.equal(_run(m, arr['x'], device, meta.get('crop')), y)  # the cached plan, bit for bit


@pytest.mark.parametrize('name', NAMES)
def test_forced_bf16_mode(device, name):
    meta, arr, sd = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = 'bf16'
    m.atd_force = _forced(meta, arr, device)
    err = (_run(m, arr['x'], device, meta.get('crop')) - arr['y']).abs().max().item()
    print(f'{name} bf16: max-abs {err:.3e}')
    assert err <= _tol(arr['y'], 3e-2)


@pytest.mark.parametrize('name', NAMES)
def test_forced_fp16_io(device, name):
    meta, arr, sd = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.atd_force = _forced(meta, arr, device)
    y = m(arr['x'].to(device).half())
    torch.cuda.synchronize()
    assert y.dtype == torch.float16
    crop = meta.get('crop')
    if crop:
        y = y[:, :, : crop[1], : crop[3]]
    err = (y.float().cpu() - arr['y']).abs().max().item()
    print(f'{name} fp16 io: max-abs {err:.3e}')
    assert err <= 2e-3 * max(1.0, arr['y'].abs().max().item()), f'{name}: {err:.3e}'


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', GUARDED)
def test_free_running_on_guarded_fixtures(device, name, precision):
    meta, arr, sd = _case(name)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    m.precision = precision
    m.atd_record = True
    y = _run(m, arr['x'], device, meta.get('crop'))
    assert len(m.atd_recorded) == meta['layers']
    for li, (ids, perm) in enumerate(m.atd_recorded):
        want = arr[f'tk_id_stable_{li}'].to(torch.int32)
        assert torch.equal(ids.cpu(), want), f'layer {li}: {(ids.cpu() != want).sum().item()} ids differ'
        assert torch.equal(perm.cpu().long(), torch.sort(ids.cpu().long(), dim=-1, stable=True).indices), li
    ref = arr['y_stable']
    err = (y - ref).abs().max().item()
    print(f'{name} {precision} free: max-abs {err:.3e}')
    assert err <= _tol(ref), err
    m.atd_record = False  # off again: the cached plan gives the same result and records nothing
    assert torch.equal(_run(m, arr['x'], device, meta.get('crop')), y) and m.atd_recorded == []


BIG = [
    (dict(embed_dim=48, depths=(2, 2), num_heads=(4, 4), window_size=16, num_tokens=64, reducted_dim=8, upscale=2, upsampler='pixelshuffledirect'), (2, 3, 96, 80)),
    (dict(embed_dim=48, depths=(3,), num_heads=(4,), window_size=8, num_tokens=64, reducted_dim=8, upscale=2, upsampler='pixelshuffledirect'), (1, 3, 61, 94)),
    (dict(embed_dim=210, depths=(2,), num_heads=(6,), window_size=16, num_tokens=128, reducted_dim=10, upscale=4, upsampler='pixelshuffle'), (1, 3, 40, 50)),
]  # fmt: skip


@pytest.mark.parametrize('kw,shape', BIG)
@pytest.mark.parametrize('precision', ['bf16x3', 'bf16'])
def test_larger_inputs_against_oracle_on_the_engine_trajectory(device, kw, shape, precision):
    sd = synth.atd_state_dict(seed=811, **kw)
    x = synth.synth_input(shape, 811)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    # (the permutation being the stable sort of the ids, and every differing id having an oracle margin below TAU, are asserted inside)
    y, _, ref, differ, total = run_on_engine_trajectory(m, sd, x, device, precision)
    y = y.float().cpu()
    assert len(m.atd_recorded) == sum(kw['depths'])
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    print(f'{kw["embed_dim"]}/{kw["window_size"]} {shape} {precision}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f}), {differ} of {total} ids differ')
    assert precision == 'bf16' or differ <= 0.002 * total
    assert err <= _tol(ref, 3e-4 if precision == 'bf16x3' else 3e-2), err


def test_upscale_uint8(device):
    meta, arr, sd = _case([n for n in NAMES if 'light_x2' in n][0])
    x = arr['x']
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (x[0].permute(1, 2, 0) * 255).round().to(torch.uint8).to(device)
    half = resselt_amd.upscale(m, img)  # fp16 tensors inside: the rounded input may move a category, so only the f32 run is compared
    assert half.dtype == torch.uint8 and tuple(half.shape) == (2 * x.shape[2], 2 * x.shape[3], 3)
    out = resselt_amd.upscale(m, img, dtype=torch.float32)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2 * x.shape[2], 2 * x.shape[3], 3)
    y = m((img.permute(2, 0, 1)[None].float() / 255).to(device))
    want = (y.clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert (out.float() - want).abs().max().item() <= 1


@pytest.mark.parametrize('shape', [(1, 3, 3, 20), (1, 3, 20, 3), (1, 4, 16, 16)])
def test_rejected_inputs_raise_before_any_launch(device, shape):
    sd = synth.atd_state_dict(seed=3)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        m(torch.rand(shape, device=device))
    torch.cuda.synchronize()
    assert L.load().rsa_check_status() == 0
