"""End-to-end GPU parity of GFISR v1 against the reference's vectors (tools/gen_golden_gfisr.py).

Tolerance: max-abs <= MODEL_REL * max(1, max|y|) in 'auto' (= 'bf16x3' for this family) and 'bf16x3', the bar of tests/test_gfisrv2_gpu.py
(imported, not copied).  'bf16' is no precision of the gated family (``precisions`` is ('bf16x3', 'fp16')): asking for it raises, as it
does for GFISRv2.  The one-product 'fp16' mode is a benchmark mode, checked at the looser bar v2's file gives it.
gfisr_x4_psd_d48_b24_9x11 is the depth check: the default 24 blocks, almost five full rotations of the Inception modules.  The two
``pixel_unshuffle`` fixtures are built directly, as the reference's loader cannot produce them.  The probe grids the reference runs (4x4,
4x5, 5x5) meet the same bar; 3x3, 3x4 and 4x3 raise as they do there.

Launches per block: ten steps and twelve kernels (a transform is two kernels) -- rsa_layernorm, fc1, the pad, the forward DFT,
rsa_gfisr_ln_spectral, the inverse DFT, the crop, rsa_gated_dwconv, fc2, rsa_group_norm_apply; five and five with ``fft_mode=False``.
"""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs.gfisr.arch import GFISR
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.utils import synth
from test_gfisrv2_gpu import MODEL_REL

pytestmark = pytest.mark.gpu

NAMES = [n for n in golden_names('gfisr_') if n != 'gfisr_probe']


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _sd(meta):
    return synth.gfisr_state_dict(seed=meta['seed'], **meta['synth'])


def _model(meta, device):
    sd = _sd(meta)
    if meta['direct']:  # a pixel_unshuffle model: no loader produces it
        m = GFISR(**meta['synth'])
        m.load_state_dict(dict(sd))
    else:
        m = resselt_amd.load_from_state_dict(dict(sd))
    return m.to(device)


def test_fixtures():
    assert len(NAMES) == 12


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = _model(meta, device)
    assert isinstance(m, GFISR) and m.resolved_precision() == 'bf16x3'
    m.precision = precision
    x = arr['x'].to(device)
    x0 = x.clone()
    y = m(x)
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} {precision}: max-abs {err:.3e} (|y|max {arr["y"].abs().max():.3f})')
    assert err <= MODEL_REL * max(1.0, arr['y'].abs().max().item()), f'{name} {precision}: max-abs {err:.3e}'
    y2 = m(x)  # second call: the cached plan
    assert torch.equal(y2, y)
    assert torch.equal(x, x0)  # the caller's input is never written


@pytest.mark.parametrize('name', NAMES)
def test_fp16_mode_runs(device, name):
    meta, arr = load_golden(name)
    m = _model(meta, device)
    m.precision = 'fp16'
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape and torch.isfinite(y).all()
    err = (y.cpu() - arr['y']).abs().max().item()
    print(f'MEASURE {name} fp16: max-abs {err:.3e}')
    assert err <= 3e-2 * max(1.0, arr['y'].abs().max().item())


def test_bf16_is_no_precision_of_the_family():
    meta, _ = load_golden('gfisr_x2_psd_d16_b6_b2_6x8')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta)))
    assert m.precisions == ('bf16x3', 'fp16')
    m.precision = 'bf16'
    with pytest.raises(ValueError, match="precision must be 'auto' or one of"):
        m.resolved_precision()


def test_a_second_input_size_through_the_same_model(device):
    """The DFT tables are per padded size: two more sizes through ONE model, alternating, each against the fp64 oracle."""
    import gfisr_oracle as O

    meta, arr = load_golden('gfisr_x2_psd_d16_b6_b2_6x8')
    sd = _sd(meta)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xs = [arr['x'], synth.synth_input((1, 3, 9, 5), 77), synth.synth_input((1, 3, 6, 7), 78)]
    with torch.no_grad():
        refs = [arr['y'].double()] + [O.gfisr_forward(sd, x.double()) for x in xs[1:]]
    first = []
    for x, ref in zip(xs, refs):
        y = m(x.to(device)).cpu()
        assert y.shape == ref.shape and (y.double() - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item())
        first.append(y)
    for x, y0 in zip(xs, first):  # and again, from the cached plans
        assert torch.equal(m(x.to(device)).cpu(), y0)


def test_launch_count(device):
    """Per block ten launch steps and twelve kernels (a transform is two); around them in_to_dim, the trunk's ``+ x`` and the head's one."""
    meta, arr = load_golden('gfisr_x2_psd_d16_b6_b2_6x8')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_gfisr_dft') == 2 * 6 and calls.count('rsa_gfisr_ln_spectral') == 6 and calls.count('rsa_plane_window') == 2 * 6
    assert calls.count('rsa_gated_dwconv') == 6 and 'rsa_gfisr_spectral' not in calls and 'rsa_gfisr_gate' not in calls
    assert m.launches_per_forward() == 12 * 6 + 3  # (the plan does not count the conversion of the caller's input into planes)
    meta, arr = load_golden('gfisr_x3_psd_d16_nofft_b5_4x3')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert m.fft_mode is False
    m(arr['x'].to(device))
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls == ['rsa_gated_dwconv'] * 5 and m.launches_per_forward() == 5 * 5 + 3


def test_probe_sizes(device):
    meta, arr = load_golden('gfisr_probe')
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    for p in meta['probe']:
        h, w = p['size']
        if p['raises'] is None:
            ref = arr[f'y_{h}x{w}']
            y = m(arr[f'x_{h}x{w}'].to(device)).cpu()
            assert y.shape == ref.shape and (y - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item()), (h, w)
        else:
            assert p['raises'] == 'RuntimeError' and 'Padding size should be less than' in p['message']
            with pytest.raises(RuntimeError, match='Padding size should be less than'):
                m(torch.rand(1, 3, h, w, device=device))


def test_upscale_with_one_tile_equals_the_plain_forward(device):
    meta, arr = load_golden('gfisr_x2_dys_d16_b2_5x7')
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

    sd = synth.gfisr_state_dict(scale=2, dim=16, n_blocks=2, seed=1440)
    x = synth.synth_input((1, 3, 7, 6), 1440)
    outs = []
    for ext in ('pth', 'safetensors'):
        p = tmp_path / f'm.{ext}'
        (torch.save(sd, p) if ext == 'pth' else save_file({k: v.contiguous() for k, v in sd.items()}, str(p)))
        m = resselt_amd.load_from_file(str(p)).to(device)
        assert m.parameters_info.upscale == 2 and m.parameters_info.name == 'GFISR'
        outs.append(m(x.to(device)).cpu())
    assert outs[0].shape == (1, 3, 14, 12) and torch.equal(outs[0], outs[1])
