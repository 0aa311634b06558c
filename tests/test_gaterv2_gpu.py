"""End-to-end GPU parity of GateRv2 against the reference's vectors (tools/gen_golden_gaterv2.py).

Tolerance: max-abs <= MODEL_REL * max(1, max|y|) in 'auto' (= 'bf16x3') and 'bf16x3', the bar of tests/test_moesr_gpu.py (imported, not
copied).  The one-product modes 'fp16' and 'bf16' run and their error is printed on a MEASURE line.  The second call (the cached plan) is
bit-equal.  The launch count of the plan is DESIGN.md section 28's table: ten kernels per MetaGated, eight per latent block (the attention is
three), two per Down, three per Up, in_to_dim, the shortcut (one at x1, the ConvBlock's three above), the head.
"""

import pytest
import torch

import gaterv2_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs.gaterv2.arch import GateRV2
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.utils import synth
from test_moesr_gpu import MODEL_REL

pytestmark = pytest.mark.gpu

NAMES = [n for n in golden_names('gaterv2_') if n != 'gaterv2_probe']


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _sd(meta):
    return synth.gaterv2_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures():
    assert len(NAMES) == 17


@pytest.mark.parametrize('precision', ['auto', 'bf16x3'])
@pytest.mark.parametrize('name', NAMES)
def test_matches_reference_vectors(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    assert isinstance(m, GateRV2) and m.resolved_precision() == 'bf16x3'
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


@pytest.mark.parametrize('precision', ['fp16', 'bf16'])
@pytest.mark.parametrize('name', NAMES)
def test_one_product_modes_run(device, name, precision):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m.precision = precision
    y = m(arr['x'].to(device))
    torch.cuda.synchronize()
    assert y.shape == arr['y'].shape and torch.isfinite(y).all()
    print(f'MEASURE {name} {precision}: max-abs {(y.cpu() - arr["y"]).abs().max().item():.3e}')


def _head_launches(m):
    if m.up is None or m.upsampler in ('pixelshuffledirect', 'conv'):
        return 1
    if m.upsampler == 'pixelshuffle':
        return 2 + 2 * (len(m.up.layers) - 2)
    return None


@pytest.mark.parametrize('name', ['gaterv2_x1_unequal_d8_l3_9x11', 'gaterv2_x1_d8_l2_chunks_45x50', 'gaterv2_x3_psd_d8_6x5', 'gaterv2_x4_ps_d16_7x4'])
def test_launch_count(device, name):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta))).to(device)
    m(arr['x'].to(device))
    mg, lat, lv = m.meta_gated_count(), m.num_latent, m.levels
    calls = [meta_['kernel'] for meta_, _ in m.last_plan().kernel_calls]
    assert calls.count('rsa_gaterv3_local_gate') == mg and calls.count('rsa_gaterv3_sca_apply') == mg
    assert calls.count('rsa_gaterv2_linear_attention') == lat
    assert calls.count('rsa_rmsnorm') == 2 * mg + lat and calls.count('rsa_gated_dwconv') == mg + lat and calls.count('rsa_pixel_unshuffle2') == lv
    table = 1 + 10 * mg + 2 * lv + 8 * lat + 3 * lv + (1 if m.scale == 1 else 3)
    assert m.expected_launches() == table
    assert m.launches_per_forward() == table + _head_launches(m)  # (the plan does not count the conversion of the caller's input into planes)


def test_other_sizes_and_dtypes_through_one_model(device):
    """Two more sizes and the half dtypes through ONE model, each against the fp64 oracle; then again from the cached plans."""
    meta, arr = load_golden('gaterv2_x2_psd_d8_5x7')
    sd = _sd(meta)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    xs = [arr['x'], synth.synth_input((1, 3, 9, 4), 77), synth.synth_input((3, 3, 3, 6), 78)]
    with torch.no_grad():
        refs = [O.gaterv2_forward(sd, x.double()) for x in xs]
    first = []
    for x, ref in zip(xs, refs):
        y = m(x.to(device)).cpu()
        assert y.shape == ref.shape and (y.double() - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item())
        first.append(y)
    for x, y0 in zip(xs, first):
        assert torch.equal(m(x.to(device)).cpu(), y0)
    for dt, bar in ((torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)):  # the parameters and the output in the half dtype: two ulps of |y| <= 2
        mh = resselt_amd.load_from_state_dict(dict(sd)).to(device).to(dt)
        sdh = {k: (v.to(dt).double() if v.is_floating_point() else v) for k, v in sd.items()}
        xh = xs[0].to(dt)
        with torch.no_grad():
            ref = O.gaterv2_forward(sdh, xh.double())
        y = mh(xh.to(device)).cpu()
        assert y.dtype == dt and ref.abs().max().item() <= 2 and (y.double() - ref).abs().max().item() <= bar


def test_the_widest_latent_stage(device):
    """A latent width of 1024 (m = 64) behind a 512-wide MetaGated level: the limits of the constructor, against the fp64 oracle."""
    kw = dict(dim=512, enc_blocks=(1,), dec_blocks=(1,), num_latent=1)
    sd = synth.gaterv2_state_dict(seed=31, **kw)
    m = GateRV2(**kw)
    m.load_state_dict(dict(sd))
    m = m.to(device)
    x = synth.synth_input((1, 3, 5, 6), 31)
    with torch.no_grad():
        ref = O.gaterv2_forward(sd, x.double())
    y = m(x.to(device)).cpu()
    err = (y.double() - ref).abs().max().item()
    print(f'MEASURE latent width 1024: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})')
    assert y.shape == ref.shape and err <= MODEL_REL * max(1.0, ref.abs().max().item())


def test_probe_sizes(device):
    meta, arr = load_golden('gaterv2_probe')
    models = {tag: resselt_amd.load_from_state_dict(dict(synth.gaterv2_state_dict(seed=meta['seed'], **kw))).to(device) for tag, kw in meta['synth'].items()}
    for p in meta['probe']:
        h, w = p['size']
        m = models[p['model']]
        if p['raises'] is None:
            key = f'{p["model"]}_{h}x{w}'
            if f'x_{key}' not in arr:
                continue
            ref = arr[f'y_{key}']
            y = m(arr[f'x_{key}'].to(device)).cpu()
            assert y.shape == ref.shape and (y - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item()), (h, w)
        else:
            assert p['raises'] == 'RuntimeError' and 'Padding size should be less than' in p['message']
            before = m.launches_per_forward()
            with pytest.raises(RuntimeError, match='Padding size should be less than'):
                m(torch.rand(1, 3, h, w, device=device))
            assert m.launches_per_forward() == before  # refused before a plan was built or anything launched


def test_the_top_left_corner_is_the_unmodified_references_output(device):
    """The reference module keeps ``scale = 1`` and returns the H x W corner of the x2 image; the engine returns the whole image."""
    meta, arr = load_golden('gaterv2_probe')
    case, _ = load_golden(meta['scale_crop']['case'])
    m = resselt_amd.load_from_state_dict(dict(_sd(case))).to(device)
    x, ref = arr['x_crop'], arr['y_crop_unmodified']
    h, w = x.shape[-2:]
    y = m(x.to(device)).cpu()
    assert y.shape[-2:] == (2 * h, 2 * w) and ref.shape[-2:] == (h, w)
    assert (y[:, :, :h, :w] - ref).abs().max().item() <= MODEL_REL * max(1.0, ref.abs().max().item())


def test_upscale_on_uint8(device):
    meta, arr = load_golden('gaterv2_x2_dys_d8_6x7')
    sd = _sd(meta)
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    img = (torch.rand(9, 11, 3, generator=torch.Generator().manual_seed(3)) * 255).to(torch.uint8)
    out = resselt_amd.upscale(m, img.to(device), dtype=torch.float32)
    with torch.no_grad():
        ref = O.gaterv2_forward(sd, (img.double() / 255).permute(2, 0, 1)[None])
    want = (ref.clamp(0, 1) * 255).round()[0].permute(1, 2, 0)
    assert out.shape == (18, 22, 3) and out.dtype == torch.uint8
    assert (out.cpu().double() - want).abs().max().item() <= 1  # within one code of the oracle's quantised output
    plain = ops.nchw_to_image_u8(m(ops.image_u8_to_nchw(img.to(device), torch.float32)))[0]
    assert torch.equal(out, plain)
    with pytest.warns(RuntimeWarning, match='normalises over the whole image'):  # sca's mean and the attention span the tensor they are given
        tiled = resselt_amd.upscale(m, img.to(device), tile=(5, 6), halo=2, dtype=torch.float32)
    assert tiled.shape == out.shape
