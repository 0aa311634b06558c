"""Real-CUGAN without a GPU: detection, inferred metadata, strict state dicts, registry order, the input sizes the reference refuses, the
tiling warning, and the plan's geometry -- a float64 replay of its layer records (arch.cugan_layers) on the same grids and windows the
kernels use, compared to the reference's vectors (tools/gen_golden_cugan.py) at the bar of test_oracle_golden.py."""

import warnings

import pytest
import torch
import torch.nn.functional as F

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs.cugan.arch import PRO_SCALE, PRO_SHIFT, cugan_layers
from resselt_amd.utils import synth

NAMES = golden_names('cugan_')


def _state_dict(meta):
    return synth.cugan_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures_exist():
    assert len(NAMES) >= 6
    variants = {load_golden(n)[0]['synth']['variant'] for n in NAMES}
    assert variants == {'2x', '3x', '4x', '2x_fast'}


@pytest.mark.parametrize('name', NAMES)
def test_claimed_with_reference_metadata(name):
    meta, _ = load_golden(name)
    sd = _state_dict(meta)
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert meta['claimed_by'] == 'CuGAN'
    assert type(m).__name__ == meta['metadata']['cls']
    assert vars(m.parameters_info) == {k: meta['metadata'][k] for k in ('in_channels', 'out_channels', 'upscale', 'name')}
    m.load_state_dict(sd, strict=True)
    assert set(m.state_dict()) == set(sd)
    assert m.is_pro == ('pro' in sd)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k


@pytest.mark.parametrize('variant', ['2x', '4x'])
def test_strict_key_set_includes_pro(variant):
    m = resselt_amd.load_from_state_dict(dict(synth.cugan_state_dict(variant, pro=True)))
    assert 'pro' in m.state_dict()
    plain = synth.cugan_state_dict(variant)
    with pytest.raises(RuntimeError, match='pro'):
        m.load_state_dict(plain, strict=True)
    sd = synth.cugan_state_dict(variant, pro=True)
    sd['unet2.extra.weight'] = torch.zeros(1)
    with pytest.raises(RuntimeError, match='extra'):
        m.load_state_dict(sd, strict=True)


def test_registry_order_follows_reference():
    from resselt_amd.archs import internal_registry

    order = list(internal_registry.store.keys())
    assert order.index('Compact') < order.index('CuGAN') < order.index('PLKSR')


@pytest.mark.parametrize('variant, ok, bad', [
    ('2x', [(20, 24), (21, 25)], [(18, 18), (19, 30), (30, 18)]),
    ('4x', [(20, 24), (21, 25)], [(18, 18)]),
    ('3x', [(18, 18), (21, 26)], [(16, 17), (14, 20)]),
    ('2x_fast', [(40, 40), (44, 44), (48, 64)], [(41, 41), (42, 46), (38, 40)]),
])  # fmt: skip
def test_minimum_sizes_match_reference(variant, ok, bad):
    for h, w in ok:
        cugan_layers(variant, 3, 3, h, w)
    for h, w in bad:
        with pytest.raises(ValueError):
            cugan_layers(variant, 3, 3, h, w)


def test_forward_refuses_small_input_before_any_launch():
    m = resselt_amd.load_from_state_dict(dict(synth.cugan_state_dict('2x')))
    with pytest.raises(ValueError):
        m._build_plan(None, None, (1, 3, 18, 18), torch.float32, m.products)


def _fake_forward(scale):
    return lambda x: F.interpolate(x, scale_factor=scale, mode='nearest')


def test_tiling_warns_for_whole_image_statistics():
    from resselt_amd.tiling import upscale_tiled

    m = resselt_amd.load_from_state_dict(dict(synth.cugan_state_dict('2x')))
    assert m.global_statistics
    m.forward = _fake_forward(2)  # the tiler's logic only: no GPU here
    x = torch.rand(1, 3, 80, 80)
    with pytest.warns(RuntimeWarning, match='whole image'):
        upscale_tiled(m, x, 2, (40, 40), halo=4, check=False)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        upscale_tiled(m, x, 2, (96, 96), halo=4, check=False)  # one tile: no warning


# ---------------------------------------------------------------------------------------------------------------- float64 replay
def replay(variant: str, sd: dict, x: torch.Tensor, pro: bool) -> torch.Tensor:
    """Execute the plan's layer records as the kernels do (3x3 convolutions zero-padded over the whole grid, the strided and transposed
    ones on their windows, SE in place on its window), in float64."""
    n, c, h0, w0 = x.shape
    g = cugan_layers(variant, 3, 3, h0, w0)
    sd = {k: v.to(torch.float64) for k, v in sd.items()}
    buf = {name: torch.zeros((n, b.channels, *g.grids[b.grid]), dtype=torch.float64) for name, b in g.bufs.items()}

    def win(t, w):
        return t[:, :, w.y0 : w.y0 + w.h, w.x0 : w.x0 + w.w]

    xi = x.to(torch.float64)
    if pro:
        xi = xi * PRO_SCALE + PRO_SHIFT
    r = g.unshuffle
    H0, W0 = g.grids['g0']
    xp = F.pad(xi, (g.pad_left, r * W0 - g.pad_left - w0, g.pad_top, r * H0 - g.pad_top - h0), mode='reflect')
    buf['x'] = F.pixel_unshuffle(xp, r) if r > 1 else xp
    for ly in g.layers:
        w, b = sd.get(f'{ly.key}.weight'), sd.get(f'{ly.key}.bias')
        if ly.op == 'conv3':
            v = F.conv2d(buf[ly.src][:, : w.shape[1]], w, b, padding=1)
            if ly.lrelu:
                v = F.leaky_relu(v, 0.1)
            if ly.res is not None:
                v = v + buf[ly.res]
            buf[ly.dst] = v
        elif ly.op == 'conv_s2':
            v = F.leaky_relu(F.conv2d(win(buf[ly.src], ly.win_in), w, b, stride=2), 0.1)
            assert v.shape[2:] == (ly.win_out.h, ly.win_out.w)
            win(buf[ly.dst], ly.win_out)[:] = v
        elif ly.op == 'deconv':
            v = F.conv_transpose2d(win(buf[ly.src], ly.win_in), w, b, stride=ly.stride, padding=ly.pad)
            assert v.shape[2:] == (ly.win_out.h, ly.win_out.w)
            if ly.lrelu:
                v = F.leaky_relu(v, 0.1)
            if ly.res is not None:
                v = v + win(buf[ly.res], ly.win_out)
            win(buf[ly.dst], ly.win_out)[:] = v
        else:
            t = win(buf[ly.src], ly.win_in)
            m = t.mean((2, 3), keepdim=True)
            hdn = F.relu(F.conv2d(m, sd[f'{ly.key}.conv1.weight'], sd[f'{ly.key}.conv1.bias']))
            gate = torch.sigmoid(F.conv2d(hdn, sd[f'{ly.key}.conv2.weight'], sd[f'{ly.key}.conv2.bias']))
            t.mul_(gate)
    oh, ow = g.out_hw
    ps = g.pixel_shuffle
    y0, x0 = g.out_origin
    m = buf[g.out_map][:, : 3 * ps * ps, y0 : y0 + -(-oh // ps), x0 : x0 + -(-ow // ps)]
    y = (F.pixel_shuffle(m, ps) if ps > 1 else m)[:, :, :oh, :ow]
    if g.base_div:
        y = y + F.interpolate(xi, scale_factor=g.base_div, mode='nearest')[:, :, :oh, :ow]
    if pro:
        y = (y - PRO_SHIFT) / PRO_SCALE
    return y


@pytest.mark.parametrize('name', NAMES)
def test_plan_replay_matches_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = _state_dict(meta)
    y = replay(meta['synth']['variant'], sd, arr['x'], meta['synth'].get('pro', False))
    ref = arr['y'].to(torch.float64)
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item(), f'{name}: max-abs {err:.3e} (|y|max {ref.abs().max():.3f})'


def test_second_down_convolution_reads_an_odd_origin():
    g = cugan_layers('2x', 3, 3, 20, 24)
    downs = [ly for ly in g.layers if ly.op == 'conv_s2']
    assert [ly.key for ly in downs] == ['unet1.conv1_down', 'unet2.conv1_down', 'unet2.conv2_down']
    assert downs[2].win_in.y0 % 2 == 1 and downs[2].win_in.x0 % 2 == 1
