"""CPU checks of the FDAT loader: detection and registry order, the inferred hyper-parameters and metadata against the reference's fixtures,
the MetaUpsample decode of every head, state_dict round trips, load-time NotImplementedError for geometries the kernels cannot run, and
the argument checks of the new C-ABI entry points (no GPU needed: they return RSA_E_ARG before any launch)."""

import ctypes as C

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.fdat.arch import FDAT, SAMPLE_MODS3
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

NAMES = golden_names('fdat_')
E_ARG, E_UNSUPPORTED = -1, -2  # RSA_E_ARG, RSA_E_UNSUPPORTED
B = dict(embed_dim=48, num_groups=1, depth_per_group=1, num_heads=4, window_size=4, mid_dim=32)


def test_fixtures_exist():
    assert len(NAMES) >= 20


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    assert meta['claimed_by'] == 'FDAT'
    sd = synth.fdat_state_dict(seed=meta['seed'], **meta['synth'])
    claims = [a.id for a in internal_registry.store.values() if a.detect(sd)]
    assert claims[0] == 'FDAT'
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, FDAT)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_and_round_trip(name):
    meta, _ = load_golden(name)
    sd = synth.fdat_state_dict(seed=meta['seed'], **meta['synth'])
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert set(got) == set(sd)
    assert not any(k.endswith('base_offset') for k in got)
    for k, v in sd.items():
        assert got[k].shape == v.shape and torch.equal(got[k].to(v.dtype), v), k
    m2 = resselt_amd.load_from_state_dict(dict(got))
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), got.values()))


def test_registry_order():
    ids = [a.id for a in internal_registry.store.values()]
    assert ids.index('MoSR') < ids.index('FDAT') < ids.index('CuGAN')


def test_other_transformers_keep_their_claimants():
    for arch, sd in (('dat', synth.dat_state_dict(embed_dim=64, depth=(2,), num_heads=(4,), split_size=(2, 4))),
                     ('RGT', synth.rgt_state_dict(embed_dim=48, depth=(2,), num_heads=(4,), split_size=(2, 4))),
                     ('MoSR', synth.mosr_state_dict(n_block=2, dim=32))):  # fmt: skip
        claims = [a.id for a in internal_registry.store.values() if a.detect(sd)]
        assert claims[0] == arch and 'FDAT' not in claims
    sd = synth.fdat_state_dict(**B)
    assert [a.id for a in internal_registry.store.values() if a.detect(sd)] == ['FDAT']


@pytest.mark.parametrize('up', SAMPLE_MODS3)
@pytest.mark.parametrize('scale', [1, 2, 3, 4])
def test_meta_upsample_decode(up, scale):
    sd = synth.fdat_state_dict(**dict(B, upsampler_type=up, scale=scale))
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert (m.head, m.scale, m.s_int, m.mid_dim) == (up, scale, scale, 32)
    meta = m.get_buffer('upsampler.MetaUpsample').tolist()
    assert meta == [3, SAMPLE_MODS3.index(up), scale, 48, 3, 32, 4]


@pytest.mark.parametrize('scale,unshuffle', [(1, 4), (2, 2)])
def test_unshuffle_reports_the_reference_scale(scale, unshuffle):
    sd = synth.fdat_state_dict(**dict(B, scale=scale, unshuffle_mod=True))
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert (m.parameters_info.upscale, m.unshuffle, m.s_int) == (scale, unshuffle, 4)


@pytest.mark.parametrize('kw,msg', [
    (dict(embed_dim=144, num_heads=4), 'head_dim'),  # 36 channels per head > 32
    (dict(embed_dim=48, num_heads=5), 'head_dim'),  # does not divide
    (dict(window_size=17), 'window'),  # 289 tokens > 256
    (dict(upsampler_type='lda', scale=2, mid_dim=40), 'mid_dim'),  # LDA: mid a multiple of 16
    (dict(upsampler_type='pa_up', scale=2, mid_dim=36), 'mid_dim'),
])  # fmt: skip
def test_unsupported_geometry_raises_at_load(kw, msg):
    sd = synth.fdat_state_dict(**dict(B, **kw))
    with pytest.raises(NotImplementedError, match=msg):
        resselt_amd.load_from_state_dict(dict(sd))


def test_embed_dim_above_interact_limit_raises():
    # (a checkpoint cannot carry it: MetaUpsample is uint8; the constructor still refuses before any launch)
    with pytest.raises(NotImplementedError, match='embed_dim 264'):
        FDAT(embed_dim=264, num_heads=12)


def test_symbols_exported():
    lib = L.load()
    for name in ('rsa_fdat_interact', 'rsa_pa_gate', 'rsa_lda_offsets', 'rsa_lda_attention'):
        assert name in L.EXPORTS and hasattr(lib, name)


def _interact(**kw):
    p = L.FdatInteractParams()
    p.batch, p.H, p.W, p.C, p.mode, p.fmt = 1, 8, 8, 48, 0, 0
    p.a_hi = p.c_hi = p.x = p.x_out = p.cm = 16
    p.a_plane_stride = p.c_plane_stride = 64
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize('kw', [dict(C=257), dict(C=0), dict(mode=2), dict(fmt=3), dict(reserved0=1), dict(cm=None), dict(x_out=None),
                                dict(a_plane_stride=10), dict(out_hi=16, gamma=None), dict(out_lo=16),
                                dict(x=None, out_hi=16, out_plane_stride=64, gamma=16, beta=16, eps=1e-5)])  # fmt: skip  (norm2 needs x)
def test_interact_argument_checks(kw):
    assert L.load().rsa_fdat_interact(C.byref(_interact(**kw)), None) == E_ARG


def test_lda_and_pa_argument_checks():
    lib = L.load()
    op = L.LdaOffsetsParams()
    op.batch, op.H, op.W, op.Hout, op.Wout, op.hidden, op.groups, op.eps = 1, 4, 4, 8, 8, 16, 3, 1e-6  # groups must be 2
    op.q_hi = op.dw_weight = op.gamma = op.beta = op.out_hi = 16
    op.q_plane_stride, op.out_plane_stride = 16, 64
    assert lib.rsa_lda_offsets(C.byref(op), None) == E_ARG
    op.groups, op.hidden = 2, 66  # hidden <= 64
    assert lib.rsa_lda_offsets(C.byref(op), None) == E_ARG
    ap = L.LdaAttnParams()
    ap.batch, ap.H, ap.W, ap.Hout, ap.Wout, ap.hidden, ap.C, ap.groups = 1, 4, 4, 8, 8, 16, 40, 2  # C a multiple of 16
    ap.q_hi = ap.k_hi = ap.v_hi = ap.offset = ap.rpb = ap.out_hi = 16
    ap.q_plane_stride = ap.k_plane_stride = ap.v_plane_stride = 16
    ap.out_plane_stride = 64
    assert lib.rsa_lda_attention(C.byref(ap), None) == E_ARG
    ap.C, ap.Hout = 32, 1  # Hout >= 2
    assert lib.rsa_lda_attention(C.byref(ap), None) == E_ARG
    assert lib.rsa_pa_gate(16, None, None, None, 64, 64, 1, 8, 8, 1, 0.2, 0, 16, None, None) == E_ARG  # no logit
    assert lib.rsa_pa_gate(16, None, 16, None, 10, 64, 1, 8, 8, 1, 0.2, 0, 16, None, None) == E_ARG  # plane stride < H*W


def test_deconv_act_check():
    """rsa_deconv refuses activations other than none / LeakyReLU / GELU, and rsa_conv_s2 refuses GELU.  That rsa_deconv accepts GELU, and
    what it computes, is test_fdat_kernels_gpu.py::test_deconv_gelu (an accepted descriptor launches, which needs a GPU)."""
    p = L.ResampleConvParams()
    p.batch, p.ksize, p.stride, p.pad, p.cin_planes, p.cout, p.products, p.fmt = 1, 4, 2, 1, 1, 8, 3, 0
    p.in_W, p.in_h, p.in_w, p.in_plane_stride = 4, 4, 4, 16
    p.out_H, p.out_W, p.out_plane_stride = 8, 8, 64
    p.act = L.ACT_MISH
    assert L.load().rsa_deconv(C.byref(p), None) == E_UNSUPPORTED
    p.ksize, p.stride, p.pad, p.act = 2, 2, 0, L.ACT_GELU
    p.out_H = p.out_W = 2
    assert L.load().rsa_conv_s2(C.byref(p), None) == E_UNSUPPORTED
