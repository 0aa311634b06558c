"""End-to-end GPU parity of GFISRv2 against the reference's vectors (tools/gen_golden_gfisrv2.py).

Tolerance: max-abs <= 2e-4 * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3', the bars of tests/test_moesr_gpu.py.  The
one-product 'fp16' mode is a benchmark mode, checked at its looser bar.  gfisrv2_x4_psd_d48_b24_9x11 is the depth check: the default 24
blocks, six full rotations of the Inception branches.  The tiny inputs the reference runs (1x2, 2x1, 1x3, 3x1) meet the same bar; 1x1
raises as it does there.
"""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs.gfisrv2.arch import GFISRV2
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

MODEL_REL = 2e-4  # whole models: max-abs <= MODEL_REL * max(1, |y|max) (test_newer_archs_sweep_gpu.py prints its errors against it)

NAMES = [n for n in golden_names('gfisrv2_') if n != 'gfisrv2_tiny_probe']


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _sd(meta):
    return synth.gfisrv2_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures():
    assert len(NAMES) == 9


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert isinstance(m, GFISRV2) and m.resolved_precision() == 'bf16x3'
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f})')
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
    assert err <= 3e-2 * max(1.0, arr['y'].abs().max().item())


def test_a_second_input_size_through_the_same_model(device):
    """The DFT tables are per (H, W): two fixtures' sizes through ONE model, alternating, each against its own reference run."""
    import gfisrv2_oracle as O

    meta, arr = load_golden('gfisrv2_x2_psd_d16_b5_b2_6x8')
    sd = _sd(meta)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xs = [arr['x'], synth.synth_input((1, 3, 9, 5), 77), synth.synth_input((1, 3, 6, 7), 78)]
    with torch.no_grad():
        refs = [arr['y'].double()] + [O.gfisrv2_forward(sd, x.double()) for x in xs[1:]]
    first = []
    for x, ref in zip(xs, refs):
        y = m(x.to(device)).cpu()
        assert y.shape == ref.shape and (y.double() - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item())
        first.append(y)
    for x, y0 in zip(xs, first):  # and again, from the cached plans
        assert torch.equal(m(x.to(device)).cpu(), y0)


def test_launch_count(device):
    """Nine launch steps, eleven kernels, per block (a transform is two kernels): rsa_rmsnorm, fc1, forward DFT, rsa_gfisr_spectral, fdc,
    inverse DFT, rsa_gfisr_gate, fc2, rsa_group_norm_apply; around them in_to_dim, the two trunk convolutions and the head's one."""
    meta, arr = load_golden('gfisrv2_x2_psd_d16_b5_b2_6x8')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_gfisr_dft') == 2 * 5 and calls.count('rsa_gfisr_spectral') == 5 and calls.count('rsa_gfisr_gate') == 5
    assert m.launches_per_forward() == 11 * 5 + 4  # (the plan does not count the conversion of the caller's input into planes)


def test_tiny_inputs(device):
    meta, arr = load_golden('gfisrv2_tiny_probe')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    for p in meta['probe']:
        h, w = p['size']
        if p['raises'] is None:
            ref = arr[f'y_{h}x{w}']
            y = m(arr[f'x_{h}x{w}'].to(device)).cpu()
            assert y.shape == ref.shape and (y - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item()), (h, w)
        else:
            with pytest.raises(RuntimeError, match='view_as_complex'):
                m(torch.rand(1, 3, h, w, device=device))


def test_upscale_with_one_tile_equals_the_plain_forward(device):
    meta, arr = load_golden('gfisrv2_x2_dys_d16_m16_b2_5x7')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    img = (torch.rand(9, 11, 3, generator=torch.Generator().manual_seed(3)) * 255).to(torch.uint8).to(device)
    out = resselt_amd.upscale(m, img, dtype=torch.float32)
    plain = ops.nchw_to_image_u8(m(ops.image_u8_to_nchw(img, torch.float32)))[0]
    assert out.shape == (18, 22, 3) and out.dtype == torch.uint8 and torch.equal(out, plain)
    assert torch.equal(resselt_amd.upscale(m, img, tile=(16, 16), dtype=torch.float32), out)  # the image fits one tile
    with pytest.warns(RuntimeWarning, match='normalises over the whole image'):  # the FourierUnit spans the tensor it is given
        tiled = resselt_amd.upscale(m, img, tile=(5, 6), halo=2, dtype=torch.float32)
    assert tiled.shape == out.shape


def test_load_from_file_pth_and_safetensors(device, tmp_path):
    pytest.importorskip('safetensors')
    from safetensors.torch import save_file

    sd = synth.gfisrv2_state_dict(scale=2, dim=16, n_blocks=2, seed=1340)
    x = synth.synth_input((1, 3, 7, 6), 1340)
    outs = []
    for ext in ('pth', 'safetensors'):
        p = tmp_path / f'm.{ext}'
        (torch.save(sd, p) if ext == 'pth' else save_file({k: v.contiguous() for k, v in sd.items()}, str(p)))
        m = resselt_amd.load_from_file(str(p)).to(device)
        assert m.parameters_info.upscale == 2 and m.parameters_info.name == 'GFISRV2'
        outs.append(m(x.to(device)).cpu())
    assert outs[0].shape == (1, 3, 14, 12) and torch.equal(outs[0], outs[1])
