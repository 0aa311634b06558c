"""CPU checks of the ATD loader: detection, registry order, the inferred hyper-parameters, tags and metadata against the reference's
fixtures, state_dict round trips, load-time NotImplementedError for what the kernels cannot run, the pack-time folds against torch, and the
new C-ABI entry points (symbols and argument checks; no GPU needed: they return an error before any launch)."""

import ctypes as C

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.atd.arch import ATD, head_planes
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

NAMES = golden_names('atd_')
E_ARG, E_UNSUPPORTED = -1, -2


def test_fixtures_exist():
    assert len(NAMES) >= 5


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    assert meta['claimed_by'] == 'ATD'
    kw = meta['synth']
    sd = synth.atd_state_dict(seed=meta['seed'], **kw)
    claims = [a.id for a in internal_registry.store.values() if a.detect(sd)]
    assert claims[0] == 'ATD'
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, ATD)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert (m.embed_dim, m.depths, m.num_heads, m.window_size) == (kw['embed_dim'], list(kw['depths']), list(kw['num_heads']), kw['window_size'])
    assert (m.num_tokens, m.reducted_dim, m.upsampler, m.upscale) == (kw['num_tokens'], kw['reducted_dim'], kw['upsampler'], kw['upscale'])
    assert m.category_size == meta['category_size']
    assert m.is_norm == kw.get('norm', True) and m.qkv_bias == kw.get('qkv_bias', True)
    assert m.tags[-3:] == [f'{m.embed_dim}dim', f'{m.window_size}w', f'{m.category_size}cat'] and (m.tags[0] == 'light') == (m.category_size == 128)


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_match_reference(name):
    meta, _ = load_golden(name)
    sd = synth.atd_state_dict(seed=meta['seed'], **meta['synth'])
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert set(got) == set(meta['state_dict'])
    assert all(list(got[k].shape) == v for k, v in meta['state_dict'].items())
    for k, v in sd.items():
        assert torch.equal(got[k], v), k


def test_registry_order():
    ids = [a.id for a in internal_registry.store.values()]
    meta, _ = load_golden('registry_claims')
    order = [u for u in meta['order'] if u in ids]
    assert 'ATD' in order and ids == order  # the reference's walk, restricted to what is built


def test_precisions():
    m = ATD(embed_dim=48, depths=(2,), num_heads=(4,))
    assert m.precisions == ('bf16x3', 'bf16') and m.resolved_precision() == 'bf16x3'


@pytest.mark.parametrize('kw', [dict(ape=True), dict(patch_size=2), dict(window_size=32), dict(embed_dim=260, num_heads=(10,)), dict(embed_dim=130, num_heads=(2,)),
                                dict(num_tokens=256), dict(reducted_dim=20), dict(category_size=512), dict(convffn_kernel_size=7)])  # fmt: skip
def test_unsupported_geometry_raises_at_load(kw):
    with pytest.raises(NotImplementedError):
        ATD(**dict(dict(embed_dim=48, depths=(2,), num_heads=(4,)), **kw))


@pytest.mark.parametrize('kw', [dict(embed_dim=210, num_heads=(6,), window_size=16, num_tokens=128, reducted_dim=10, category_size=256),
                                dict(embed_dim=48, num_heads=(4,), window_size=16, num_tokens=64, reducted_dim=8, category_size=128),
                                dict(embed_dim=256, num_heads=(4,), window_size=8, num_tokens=128, reducted_dim=16)])  # fmt: skip
def test_released_shapes_load(kw):
    ATD(depths=(2,), **kw)


def test_pack_folds_match_torch():
    """Head width 35: the regrouped qkv and the concatenated projections reproduce the Linear layers on random inputs."""
    torch.manual_seed(0)
    kw = dict(embed_dim=210, depths=(2,), num_heads=(6,), window_size=16, num_tokens=128, reducted_dim=10, upscale=4, upsampler='pixelshuffle')
    sd = synth.atd_state_dict(seed=5, **kw)
    m = resselt_amd.load_from_state_dict(dict(sd))
    b = 'layers.0.residual_group.layers.0'
    t = m.pack_layer(sd, b, 6, False)
    hp = head_planes(210, 6)
    assert hp == 5
    x = torch.randn(7, 210)
    wq, bq = t['wqkv']
    got = (x @ wq.t() + bq).view(7, 3, 6, 8 * hp)
    want = torch.nn.functional.linear(x, sd[f'{b}.wqkv.weight'], sd[f'{b}.wqkv.bias']).view(7, 3, 6, 35)
    assert torch.allclose(got[..., :35], want, atol=1e-6) and got[..., 35:].abs().max() == 0
    ow, oa = torch.randn(7, 6, 35), torch.randn(7, 6, 35)
    cat = torch.zeros(7, 2, 6, 8 * hp)
    cat[:, 0, :, :35], cat[:, 1, :, :35] = ow, oa
    wp, bp = t['proj']
    got = cat.reshape(7, -1) @ wp.t() + bp
    F = torch.nn.functional
    want = F.linear(ow.reshape(7, 210), sd[f'{b}.attn_win.proj.weight'], sd[f'{b}.attn_win.proj.bias']) + F.linear(
        oa.reshape(7, 210), sd[f'{b}.attn_aca.proj.weight'], sd[f'{b}.attn_aca.proj.bias'])  # fmt: skip
    assert torch.allclose(got, want, atol=1e-5)
    assert torch.equal(t['bias_table'], sd[f'{b}.attn_win.relative_position_bias_table'].t())
    s = sd[f'{b}.attn_atd.scale']
    assert torch.allclose(t['ca_scale'], 1 + s.clamp(0, 1) * torch.log(torch.tensor(128.0)))
    assert abs(t['aca_scale'] - float(sd[f'{b}.attn_aca.logit_scale'].clamp(max=4.6051702).exp())) < 1e-5


def test_capi_symbols():
    lib = L.load()
    for name in ('rsa_atd_dict', 'rsa_atd_ca', 'rsa_atd_sort', 'rsa_atd_sort_workspace_bytes', 'rsa_atd_attention', 'rsa_atd_dwconv',
                 'rsa_atd_refine', 'rsa_atd_refine_workspace_bytes'):  # fmt: skip
        assert name in L.EXPORTS and hasattr(lib, name)


def _attn(**kw):
    p = L.AtdAttnParams()
    p.batch, p.H, p.W, p.heads, p.head_dim, p.mode, p.ws, p.shift, p.gs, p.products, p.scale = 1, 16, 16, 4, 12, 0, 8, 0, 128, 1, 1.0
    p.qkv_hi, p.qkv_plane_stride, p.qkv_batch_stride = 4096, 256, 256 * 24
    p.out_hi, p.out_plane_stride, p.out_batch_stride = 4096, 256, 256 * 8
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize('kw,rc', [(dict(H=12), E_ARG), (dict(ws=17), E_ARG), (dict(shift=8), E_ARG), (dict(head_dim=65), E_UNSUPPORTED),
                                   (dict(mode=2), E_ARG), (dict(mode=1), E_ARG), (dict(mode=1, perm=4096, gs=257), E_ARG), (dict(products=2), E_UNSUPPORTED),
                                   (dict(products=3), E_ARG), (dict(qkv_plane_stride=100), E_ARG), (dict(reserved0=1), E_ARG)])  # fmt: skip
def test_attention_rejects(kw, rc):
    assert L.load().rsa_atd_attention(C.byref(_attn(**kw)), None) == rc


def test_other_entry_points_reject():
    lib = L.load()
    assert lib.rsa_atd_sort(4096, 1, 100, 129, 4096, 4096, 4096, None) == E_UNSUPPORTED
    assert lib.rsa_atd_sort(None, 1, 100, 64, 4096, 4096, 4096, None) == E_ARG
    assert lib.rsa_atd_sort_workspace_bytes(2, 5000) == 2 * 3 * 128 * 4
    c = L.AtdCaParams()
    c.batch, c.H, c.W, c.C, c.m, c.rc, c.products = 1, 8, 8, 48, 64, 17, 3
    assert lib.rsa_atd_ca(C.byref(c), None) == E_UNSUPPORTED
    c.rc = 8
    assert lib.rsa_atd_ca(C.byref(c), None) == E_ARG  # null pointers
    r = L.AtdRefineParams()
    r.batch, r.H, r.W, r.C, r.m, r.eps = 1, 8, 8, 300, 64, 1e-5
    assert lib.rsa_atd_refine(C.byref(r), None) == E_UNSUPPORTED
    assert lib.rsa_atd_refine_workspace_bytes(1, 8, 8, 300, 64) == 0
