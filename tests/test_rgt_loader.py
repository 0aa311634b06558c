"""CPU checks of the RGT loader and pack-time folds: detection (RGT, not DAT) and registry order, the inferred hyper-parameters and
metadata against the reference's fixtures, load-time NotImplementedError for geometries the kernels cannot run, the position-bias and
q-scale folds, the CPE fold, and the plain-torch oracle (tests/rgt_oracle.py) pinned to every tests/golden/rgt_*.npz fixture."""

import math

import pytest
import torch
import torch.nn.functional as F

import resselt_amd
import rgt_oracle as O
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.rgt.arch import RGT, rg_scale, rg_times
from resselt_amd.engine.transformer import HEAD_PAD
from resselt_amd.utils import synth

NAMES = golden_names('rgt_')


def _kw(meta):
    return {k: tuple(v) if isinstance(v, list) else v for k, v in meta['synth'].items()}


def test_fixtures_exist():
    assert len(NAMES) >= 7


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    assert meta['claimed_by'] == 'RGT'
    sd = synth.rgt_state_dict(seed=meta['seed'], **_kw(meta))
    claims = [a.id for a in internal_registry.store.values() if a.detect(sd)]
    assert claims[0] == 'RGT'
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, RGT)
    pi = m.parameters_info
    md = meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])


def test_registry_order():
    ids = [a.id for a in internal_registry.store.values()]
    assert ids.index('Compact') < ids.index('RGT') < ids.index('MoSR')


def test_dat_is_not_claimed_as_rgt():
    sd = synth.dat_state_dict(embed_dim=64, depth=(2,), num_heads=(4,), split_size=(2, 4))
    assert not any(a.id == 'RGT' and a.detect(sd) for a in internal_registry.store.values())
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ == 'DAT'


@pytest.mark.parametrize('kw,expect', [
    (dict(embed_dim=48, depth=(2, 2), num_heads=(4, 2), split_size=(4, 8), resi='3conv', qkv_bias=False, upscale=4),
     dict(split_size=[4, 8], depth=[2, 2], num_heads=[4, 2], resi='3conv', qkv_bias=False, upscale=4, c_ratio=0.5, hidden=96)),
    (dict(embed_dim=48, depth=(3,), num_heads=(4,), split_size=(8, 32), c_ratio=0.75, upscale=3, mlp_ratio=4.0),
     dict(split_size=[8, 32], depth=[3], num_heads=[4], resi='1conv', qkv_bias=True, upscale=3, c_ratio=0.75, hidden=192)),
    (dict(in_chans=1, embed_dim=64, depth=(1,), num_heads=(4,), split_size=(4, 4), upscale=8),
     dict(split_size=[4, 4], depth=[1], num_heads=[4], resi='1conv', qkv_bias=True, upscale=8, c_ratio=0.5, hidden=128, in_chans=1)),
])  # fmt: skip
def test_inferred_hyperparameters(kw, expect):
    m = resselt_amd.load_from_state_dict(dict(synth.rgt_state_dict(**kw)))
    got = dict(split_size=m.split_size, depth=m.depth, num_heads=m.num_heads, resi=m.resi, qkv_bias=m.qkv_bias, upscale=m.upscale, c_ratio=m.c_ratio,
               hidden=m.hidden, in_chans=m.in_chans)  # fmt: skip
    assert got == dict(dict(in_chans=3), **expect)


@pytest.mark.parametrize('kw,what', [
    (dict(embed_dim=48, num_heads=(3,)), 'even head count'),
    (dict(embed_dim=128, num_heads=(2,)), 'head_dim'),
    (dict(embed_dim=40, num_heads=(4,), c_ratio=0.25), 'RG-SA'),  # cr 10 over 4 heads
    (dict(embed_dim=48, num_heads=(4,), split_size=(16, 32)), 'split_size'),
])  # fmt: skip
def test_unsupported_geometry_raises_at_load(kw, what):
    with pytest.raises(NotImplementedError, match=what):
        RGT(depth=(2,), **kw)


def test_recursion_count_and_scale():
    assert rg_times(512, 512) == 2 and (512 // 4 ** rg_times(512, 512)) ** 2 == 1024
    assert rg_times(64, 1024) == 3 and rg_times(2160, 3840) == 3 and (2160 // 64) * (3840 // 64) == 1980
    assert rg_times(1080, 1920) == 3 and (1080 // 64) * (1920 // 64) == 480
    with pytest.raises(ValueError):
        rg_times(15, 100)
    for h in range(16, 5000, 37):
        for w in (16, 100, 4097):
            t = rg_times(h, w)
            assert (h // 4**t) <= 63 and (w // 4**t) <= 63
    assert rg_scale(180, 6, 0.5) == (30 * 0.5) ** -0.5


def _model(**kw):
    m = resselt_amd.load_from_state_dict(dict(synth.rgt_state_dict(seed=7, **kw)))
    return m, m._pack('cpu', m.products)


def test_q_scale_fold_and_cpe_fold():
    m, W = _model(embed_dim=48, depth=(2,), num_heads=(4,), split_size=(2, 4), c_ratio=0.75)
    sd = m.state_dict()
    a = 'layers.0.blocks.1.attn'
    f = m._pack_rg({k: v.float() for k, v in sd.items()}, a, 4, 'cpu')
    wq, bq = f[f'{a}.q']
    dq = 36 // 4
    scale = (48 // 4 * 0.75) ** -0.5
    x = torch.randn(5, 48)
    ref = F.linear(x, sd[f'{a}.q.weight'], sd[f'{a}.q.bias']) * scale
    got = F.linear(x, wq, bq).reshape(5, 4, HEAD_PAD)
    assert torch.allclose(got[:, :, :dq].reshape(5, 36), ref, atol=1e-5)
    assert got[:, :, dq:].abs().max() == 0
    cw, cb = f[f'{a}.cpe']
    v = torch.randn(1, 48, 5, 6)
    ref = v + F.conv2d(v, sd[f'{a}.cpe.weight'], sd[f'{a}.cpe.bias'], padding=1, groups=48)
    vp = torch.zeros(1, 4, HEAD_PAD, 5, 6)
    vp[:, :, :12] = v.reshape(1, 4, 12, 5, 6)
    got = F.conv2d(vp.reshape(1, 128, 5, 6), cw.reshape(128, 1, 3, 3), cb, padding=1, groups=128).reshape(1, 4, HEAD_PAD, 5, 6)
    assert torch.allclose(got[:, :, :12].reshape(1, 48, 5, 6), ref, atol=1e-5)


def test_position_bias_fold():
    m, W = _model(embed_dim=48, depth=(2,), num_heads=(4,), split_size=(2, 4))
    sd = {k: v.float() for k, v in m.state_dict().items()}
    for idx, (hs, ws) in enumerate(((2, 4), (4, 2))):
        dense = O._pos_bias(sd, f'layers.0.blocks.0.attn.attns.{idx}', hs, ws)  # [heads/2, N, N]
        frag = W[f'layers.0.blocks.0.attn.bias{idx}']  # [heads][1][1][64][16], S^T order
        lane = torch.arange(64)[:, None]
        r = torch.arange(16)[None, :]
        q, k = lane & 31, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        n = hs * ws
        for h in range(2):
            g = frag[h, 0, 0]
            live = (q < n) & (k < n)
            assert torch.allclose(g[live], dense[h][q.expand(64, 16)[live], k.expand(64, 16)[live]], atol=1e-6)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_fixture(name):
    meta, arr = load_golden(name)
    kw = _kw(meta)
    sd = synth.rgt_state_dict(seed=meta['seed'], **kw)
    x = arr['x'] if 'x' in arr else arr['x_u8'].float() / 255
    ref = arr['y'] if 'y' in arr else arr['y_crop']
    with torch.no_grad():
        y = O.rgt_forward(sd, x, kw['split_size'], kw['num_heads'], kw.get('c_ratio', 0.5))
    if 'y_crop' in arr:
        c = meta['crop']
        y = y[:, :, c[0] : c[1], c[2] : c[3]]
    assert (y - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


def test_fixture_sizes():
    import os

    from helpers import GOLDEN

    sizes = [os.path.getsize(os.path.join(GOLDEN, n + '.npz')) for n in NAMES]
    assert max(sizes) < 512 * 1024 and sum(sizes) < 2 * 1024 * 1024
