"""CPU checks of the RHA loader: detection, its place behind the registry's ordered walk, the inferred hyper-parameters and metadata against the reference's fixtures,
the parameter tree against the reference module's state_dict, that no other architecture's checkpoint changes owner, the load-time
NotImplementedErrors, the multiply-accumulate count against a hand count, and that the stored ``conv5x5_reparam`` pair never reaches a
packed tensor."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.rha.arch import RHA, pack_hybrid
from resselt_amd.archs.rtmosr.arch import fold_omnishift
from resselt_amd.utils import synth

NAMES = golden_names('rha_')


def _sd(meta):
    kw = dict(meta['synth'])
    kw['down_list'] = tuple(kw['down_list'])
    return synth.rha_state_dict(seed=meta['seed'], **kw)


def test_fixtures_exist():
    assert len(NAMES) == 6
    metas = [load_golden(n)[0] for n in NAMES]
    assert all(m['mode'] == 'eval' and m['claimed_by'] == 'RHA' for m in metas)
    assert {m['hyper']['head'] for m in metas} == {'conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample'}
    assert {m['hyper']['pad'] for m in metas} == {4, 8, 16, 32, 64}
    assert {d for m in metas for d in m['hyper']['down_list']} == {1, 2, 4, 8}


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    claims = [a.id for a in internal_registry if a.detect(sd)]
    assert claims == ['RHA']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, RHA)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'RHA'
    hy = meta['hyper']
    assert (m.dim, m.in_ch, m.group_blocks, m.res_blocks, m.hidden, m.window_size) == (hy['dim'], hy['in_ch'], hy['group_blocks'], hy['res_blocks'], hy['hidden'], hy['window_size'])
    assert [m.down(g) for g in range(m.group_blocks)] == hy['down_list']
    assert (m.head, m.scale, m.out_ch, m.mid_dim, m.pad) == (hy['head'], hy['scale'], hy['out_ch'], hy['mid_dim'], hy['pad'])
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'bf16', 'fp16')


@pytest.mark.parametrize('name', NAMES)
def test_parameter_tree_equals_the_reference_modules(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert list(sd) == list(meta['state_dict']) and {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert list(got) == list(meta['state_dict'])  # names and registration order of the reference module
    assert all(list(got[k].shape) == v for k, v in meta['state_dict'].items())
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'body.0.body.0.conv.att.2.scale'})
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)))


def test_detection_keys():
    arch = internal_registry.get('RHA')
    sd = synth.rha_state_dict(dim=16, group_blocks=1, res_blocks=1, down_list=(1,), window_size=4)
    assert arch.detect(sd)
    b = 'body.0.body.0'
    for drop in ('body.0.down_sample', f'{b}.norm.bias', f'{b}.fc1.weight', f'{b}.conv.att.2.scale', f'{b}.conv.att.2.positional_encoding', f'{b}.conv.att.2.dwc.bias',
                 f'{b}.conv.conv.alpha3', f'{b}.conv.conv.conv5x5_reparam.weight', f'{b}.conv.aggr.0.bias', f'{b}.fc2.bias', 'to_img.MetaUpsample'):  # fmt: skip
        assert not arch.detect({k: v for k, v in sd.items() if k != drop}), drop


def test_registry_position():
    """RHA is consulted after the ordered walk, which stays the reference's walk restricted to what it holds; the registry as a whole
    knows RHA by id, iterates over it last and counts it."""
    ids = list(internal_registry.store)
    meta, _ = load_golden('registry_claims')
    assert 'RHA' in meta['order'] and ids == [u for u in meta['order'] if u in ids] and 'RHA' not in ids
    assert list(internal_registry.late) == ['RHA'] and 'RHA' in internal_registry and internal_registry.get('RHA').id == 'RHA'
    assert [a.id for a in internal_registry] == ids + ['RHA'] and len(internal_registry) == len(ids) + 1
    assert resselt_amd.get('RHA') is internal_registry.late['RHA']
    with pytest.raises(KeyError):
        internal_registry.get('no-such-architecture')


OTHERS = [
    ('eimn', lambda: synth.eimn_state_dict(num_stages=1)), ('ESRGAN', lambda: synth.rrdbnet_state_dict(nb=1)), ('spanplus', lambda: synth.spanplus_state_dict(blocks=(1,))),
    ('SPAN', lambda: synth.span_state_dict()), ('SwinIR', lambda: synth.swinir_state_dict()), ('Compact', lambda: synth.compact_state_dict(num_conv=2)),
    ('dat', lambda: synth.dat_state_dict()), ('SpanPP', lambda: synth.spanpp_state_dict()), ('HAT', lambda: synth.hat_state_dict()),
    ('RTMoSR', lambda: synth.rtmosr_state_dict()), ('DRCT', lambda: synth.drct_state_dict()), ('PLKSR', lambda: synth.plksr_state_dict()),
    ('PLKSR', lambda: synth.realplksr_state_dict()), ('CuGAN', lambda: synth.cugan_state_dict()), ('MoSR', lambda: synth.mosr_state_dict(n_block=1)),
    ('MoSRv2', lambda: synth.mosrv2_state_dict(n_block=1)), ('RGT', lambda: synth.rgt_state_dict()), ('FDAT', lambda: synth.fdat_state_dict()),
    ('OmniSR', lambda: synth.omnisr_state_dict()), ('ATD', lambda: synth.atd_state_dict()), ('RCAN', lambda: synth.rcan_state_dict(n_resgroups=1, n_resblocks=1)),
    ('GateR', lambda: synth.gater_state_dict(dim=24, num_blocks=(1,) * 7)),
]  # fmt: skip


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('RHA').detect(sd)
    claims = [a.id for a in internal_registry if a.detect(sd)]
    assert claims and claims[0] == uid and 'RHA' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'RHA'


def test_every_other_registered_architecture_has_a_checkpoint_above():
    assert {a.id for a in internal_registry} - {'RHA'} == {u for u, _ in OTHERS}


def test_load_time_not_implemented():
    small = dict(group_blocks=1, res_blocks=1)
    with pytest.raises(NotImplementedError, match='unshuffle'):
        resselt_amd.load_from_state_dict(dict(synth.rha_state_dict(dim=16, **small), unshuffle=torch.tensor(2, dtype=torch.uint8)))
    with pytest.raises(NotImplementedError, match='multiple of 16 from 16 to 64'):
        resselt_amd.load_from_state_dict(dict(synth.rha_state_dict(dim=80, **small)))
    with pytest.raises(NotImplementedError, match='multiple of 16'):
        RHA(dim=24)
    with pytest.raises(NotImplementedError, match='window_size'):
        resselt_amd.load_from_state_dict(dict(synth.rha_state_dict(dim=16, window_size=6, **small)))
    with pytest.raises(NotImplementedError, match='down_list'):
        resselt_amd.load_from_state_dict(dict(synth.rha_state_dict(dim=16, down_list=(2, 3), group_blocks=2, res_blocks=1)))
    with pytest.raises(NotImplementedError, match='hidden'):
        RHA(dim=32, expansion_ratio=1.1)  # 35: not a multiple of 8
    with pytest.raises(NotImplementedError, match='hidden'):
        RHA(dim=32, expansion_ratio=0.75)
    with pytest.raises(NotImplementedError, match='input channels'):
        RHA(dim=32, in_ch=9)
    m = resselt_amd.load_from_state_dict(dict(synth.rha_state_dict(dim=64, in_ch=8, out_ch=2, down_list=(8, 1), window_size=4, expansion_ratio=1.0, **small)))
    assert (m.dim, m.hidden, m.in_ch, m.out_ch, m.pad) == (64, 64, 8, 2, 32)  # the limits themselves load


def test_hidden_comes_from_the_checkpoint():
    for dim, ratio in ((48, 1.5), (32, 2.0), (16, 1.0), (64, 1.125)):
        m = resselt_amd.load_from_state_dict(dict(synth.rha_state_dict(dim=dim, expansion_ratio=ratio, group_blocks=1, res_blocks=1)))
        assert m.hidden == int(ratio * dim)


def test_macs_against_a_hand_count():
    """dim 32 (C2 16, head dimension 2), hidden 48, groups pooling by 2 and by 1, two blocks each, x2 pixelshuffledirect, RGB."""
    m = resselt_amd.load_from_state_dict(dict(_sd(load_golden('rha_x2_psd_d32_dn21_g2b2_13x18')[0])))
    att = 3 * 16 * 16 + 2 * 16 * 2 + 25 * 16 + 16 * 16  # qkv, k^T v and q kv, the 5x5 of v, proj: per pooled pixel
    block = 9 * 32 * 96 + 25 * 16 + 32 * 32 + 9 * 48 * 32  # fc1, OmniShift(x1), aggr, fc2: per pixel
    tail = 25 * 32 + 32 * 32
    want = 9 * 3 * 32 + (2 * (block + att // 4) + tail) + (2 * (block + att) + tail) + 9 * 32 * 3 * 4
    assert want == 183272 and m.macs_per_input_pixel() == want
    # the attention at its own resolution: pooling by 8 leaves 1 / 64 of it
    a = RHA(dim=32, down_list=(1,), group_blocks=1, res_blocks=1).macs_per_input_pixel()
    b = RHA(dim=32, down_list=(8,), group_blocks=1, res_blocks=1).macs_per_input_pixel()
    assert a - b == att - att // 64


def test_stored_reparam_kernel_has_no_influence():
    sd = synth.rha_state_dict(dim=32, group_blocks=1, res_blocks=1, seed=3)
    other = dict(sd)
    for k in sd:
        if 'conv5x5_reparam' in k:
            other[k] = torch.full_like(sd[k], 7.0)
    key = 'body.0.body.0.conv'
    a, b = pack_hybrid(sd, key, 16, 8), pack_hybrid(other, key, 16, 8)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(u, v) for u, v in zip(fold_omnishift(sd, 'body.0.body.1'), fold_omnishift(other, 'body.0.body.1')))
    # and the packed kernel is the fold of the training parameters, not the stored pair
    w = a['omni_w'].reshape(16, 1, 5, 5)
    assert not torch.allclose(w, sd[f'{key}.conv.conv5x5_reparam.weight'])
    want = sd[f'{key}.conv.alpha4'].reshape(16, 1, 1, 1) * sd[f'{key}.conv.conv5x5.weight']
    assert torch.allclose(w[:, :, 0, 0], want[:, :, 0, 0], atol=1e-6)  # a corner tap: only the 5x5 branch reaches it
    assert sorted(a) == ['bproj', 'bqkv', 'dwb', 'dww', 'isc', 'omni_b', 'omni_w', 'pos_t', 'wproj_t', 'wqkv_t']
    sp = torch.nn.functional.softplus(sd[f'{key}.att.2.scale'].double().reshape(-1))
    assert torch.equal(a['isc'], (1.0 / sp).float()) and a['pos_t'].shape == (16, 64) and a['wqkv_t'].shape == (16, 48)
