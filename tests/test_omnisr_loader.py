"""CPU checks of the OmniSR loader: detection and registry order, the inferred hyper-parameters and metadata against the reference's
fixtures, junk-key removal, state_dict round trips, load-time NotImplementedError for geometries the kernels cannot run, and the argument
checks of the new C-ABI entry points (no GPU needed: they return an error before any launch)."""

import ctypes as C

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.omnisr.arch import OmniSR
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

NAMES = golden_names('omnisr_')
E_ARG, E_UNSUPPORTED = -1, -2  # RSA_E_ARG, RSA_E_UNSUPPORTED


def test_fixtures_exist():
    assert len(NAMES) >= 9


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    assert meta['claimed_by'] == 'OmniSR'
    sd = synth.omnisr_state_dict(seed=meta['seed'], **meta['synth'])
    claims = [a.id for a in internal_registry.store.values() if a.detect(sd)]
    assert claims[0] == 'OmniSR'
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, OmniSR)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    kw = meta['synth']
    assert (m.dim, m.res_num, m.block_num, m.pe, m.ws, m.bias) == (kw['num_feat'], kw['res_num'], kw['block_num'], kw['pe'], kw['window_size'], kw['bias'])


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_match_reference(name):
    meta, _ = load_golden(name)
    sd = synth.omnisr_state_dict(seed=meta['seed'], **meta['synth'])
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert list(got) == list(meta['state_dict'])  # names and registration order of the reference module
    assert all(list(got[k].shape) == v for k, v in meta['state_dict'].items())
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    m2 = resselt_amd.load_from_state_dict(dict(got))
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), got.values()))


def test_junk_keys_are_removed():
    sd = dict(synth.omnisr_state_dict(num_feat=32, window_size=4, up_scale=2))
    sd['total_ops'] = torch.zeros(1)
    sd['residual_layer.0.esa.total_params'] = torch.zeros(1)
    m = resselt_amd.load_from_state_dict(sd)
    assert isinstance(m, OmniSR)
    assert 'total_ops' not in sd and 'residual_layer.0.esa.total_params' not in sd


def test_window_size_without_table_is_8():
    sd = synth.omnisr_state_dict(num_feat=32, window_size=8, pe=False, up_scale=2)
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert (m.ws, m.pe) == (8, False)


def test_strict_load_rejects_missing_and_extra_keys():
    sd = synth.omnisr_state_dict(num_feat=32, window_size=4, up_scale=2)
    m = OmniSR(num_feat=32, window_size=4, up_scale=2)
    m.load_state_dict(sd)
    bad = dict(sd)
    bad.pop('output.bias')
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)))


def test_registry_order():
    ids = [a.id for a in internal_registry.store.values()]
    assert ids.index('RGT') < ids.index('OmniSR') < ids.index('MoSR')


def test_precisions():
    m = OmniSR(num_feat=32, window_size=4)
    assert m.precisions == ('bf16x3', 'bf16')
    assert m.resolved_precision() == 'bf16x3'


@pytest.mark.parametrize('kw', [dict(num_feat=132), dict(num_feat=30), dict(num_feat=64, window_size=9), dict(num_feat=64, window_size=16)])
def test_unsupported_geometry_raises_at_load(kw):
    with pytest.raises(NotImplementedError):
        OmniSR(**kw)


@pytest.mark.parametrize('c', [32, 44, 48, 64, 96, 128])
def test_supported_widths_load(c):
    OmniSR(num_feat=c, window_size=4)
    OmniSR(num_feat=c, window_size=8)


# ---------------------------------------------------------------- C-ABI argument checks (no launch happens)
def _attn(**kw):
    p = L.OmniAttnParams()
    p.batch, p.H, p.W, p.ws, p.heads, p.head_dim, p.grid, p.fmt = 1, 16, 16, 8, 4, 16, 0, 0
    p.qkv_hi, p.qkv_plane_stride, p.qkv_batch_stride = 4096, 256, 256 * 24  # 3 x 4 heads x 2 planes
    p.out_hi, p.out_plane_stride, p.out_batch_stride = 4096, 256, 256 * 8
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_capi_symbols():
    lib = L.load()
    for name in ('rsa_omni_window_attention', 'rsa_omni_channel_attention', 'rsa_omni_channel_attn_workspace_bytes', 'rsa_gelu_gate_dwconv',
                 'rsa_omni_gate_scale', 'rsa_esa_conv3x3', 'rsa_esa_maxpool', 'rsa_esa_apply'):  # fmt: skip
        assert name in L.EXPORTS and hasattr(lib, name)


@pytest.mark.parametrize('kw,rc', [(dict(H=12), E_ARG), (dict(grid=2), E_ARG), (dict(head_dim=33), E_UNSUPPORTED), (dict(heads=9), E_UNSUPPORTED),
                                   (dict(ws=16, H=16, W=16), E_UNSUPPORTED), (dict(fmt=7), E_ARG), (dict(qkv_hi=None), E_ARG),
                                   (dict(temperature=4096), E_ARG), (dict(qkv_plane_stride=100), E_ARG), (dict(batch=0), E_ARG)])  # fmt: skip
def test_window_attention_rejects(kw, rc):
    assert L.load().rsa_omni_window_attention(C.byref(_attn(**kw)), None) == rc


@pytest.mark.parametrize('kw', [dict(), dict(temperature=4096, grid=1), dict(workspace=4096), dict(temperature=4096, workspace=4096, bias_table=4096),
                                dict(temperature=4096, workspace=4096, W=20)])  # fmt: skip
def test_channel_attention_rejects(kw):
    assert L.load().rsa_omni_channel_attention(C.byref(_attn(**kw)), None) == E_ARG


def test_channel_attention_workspace():
    lib = L.load()
    assert lib.rsa_omni_channel_attn_workspace_bytes(1, 16, 16, 8, 4, 16, 0) == 0  # window mode: one launch per window, no workspace
    # grid mode: 64 residue classes x 4 heads, one 64-token chunk each: partial Gram matrices and norms, then the d x d matrices
    assert lib.rsa_omni_channel_attn_workspace_bytes(1, 16, 16, 8, 4, 16, 1) == (64 * 4 * 1 * (256 + 32) + 64 * 4 * 256) * 4
    assert lib.rsa_omni_channel_attn_workspace_bytes(1, 16, 20, 8, 4, 16, 0) == E_ARG
    assert lib.rsa_omni_channel_attn_workspace_bytes(1, 16, 16, 8, 4, 16, 3) == E_ARG


def test_gelu_gate_dwconv_rejects():
    lib = L.load()
    p = L.GeluGateDwConvParams()
    p.batch, p.H, p.W, p.planes = 1, 4, 4, 1
    p.in_hi, p.in_plane_stride, p.in_batch_stride, p.weight = 4096, 16, 32, 4096
    p.out_hi, p.out_plane_stride, p.out_batch_stride = 4096, 16, 16
    p.reserved0 = 1
    assert lib.rsa_gelu_gate_dwconv(C.byref(p), None) == E_ARG
    p.reserved0, p.in_batch_stride = 0, 16  # two input planes need 32
    assert lib.rsa_gelu_gate_dwconv(C.byref(p), None) == E_ARG
    p.in_batch_stride, p.weight = 32, None
    assert lib.rsa_gelu_gate_dwconv(C.byref(p), None) == E_ARG


def test_gate_scale_and_channel_gate_reject():
    lib = L.load()
    assert lib.rsa_omni_gate_scale(4096, None, 16, 16, 1, 4, 4, 1, None, 0, 4096, None, None) == E_ARG
    assert lib.rsa_omni_gate_scale(4096, 4096, 16, 16, 1, 4, 4, 1, 4096, 0, 4096, None, None) == E_ARG
    gp = L.ChannelGateParams()
    gp.batch, gp.H, gp.W, gp.planes, gp.hidden, gp.relu = 1, 4, 4, 1, 2, 4
    gp.in_hi, gp.w1, gp.b1, gp.w2, gp.b2, gp.workspace, gp.gate = (4096,) * 7
    assert lib.rsa_channel_gate(C.byref(gp), None) == E_ARG


def test_esa_entry_points_reject():
    lib = L.load()
    p = L.EsaConvParams()
    p.batch, p.H, p.W, p.Hout, p.Wout, p.cin, p.cout, p.stride, p.pad = 1, 15, 15, 7, 7, 16, 16, 2, 0
    p.in_, p.weight, p.bias, p.out = 4096, 4096, 4096, 4096
    p.Hout = 8
    assert lib.rsa_esa_conv3x3(C.byref(p), None) == E_ARG
    p.Hout, p.stride = 7, 3
    assert lib.rsa_esa_conv3x3(C.byref(p), None) == E_UNSUPPORTED
    p.stride, p.cin = 2, 65
    assert lib.rsa_esa_conv3x3(C.byref(p), None) == E_ARG
    assert lib.rsa_esa_maxpool(4096, 1, 16, 6, 9, 4096, None) == E_ARG
    a = L.EsaApplyParams()
    a.batch, a.H, a.W, a.C, a.f, a.Hc, a.Wc = 1, 16, 16, 64, 33, 1, 1
    a.x, a.c1, a.c3, a.wf, a.bf, a.w4, a.b4, a.out = (4096,) * 8
    assert lib.rsa_esa_apply(C.byref(a), None) == E_ARG
    a.f, a.C = 16, 129
    assert lib.rsa_esa_apply(C.byref(a), None) == E_ARG
