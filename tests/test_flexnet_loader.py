"""CPU checks of the FlexNet loader: detection, its place behind the registry's walk, the inferred hyper-parameters and metadata against the
reference's fixtures, the parameter tree against the reference module's state_dict, that no other architecture's checkpoint changes owner,
the two load-time refusals, the one deliberate difference from the reference's loader (``hidden_rate`` read from ``t_blocks.0``), that the
stored ``conv5x5_reparam`` never reaches a packed tensor, the folds, and the file round trip."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.flexnet.arch import RMS_EPS, FlexNet, fold_block, fold_omnishift
from resselt_amd.utils import synth

NAMES = golden_names('flexnet_')
ONE_BLOCK_FIRST = 'flexnet_x3_nc_d32_b12_10x12'


def _sd(meta):
    kw = dict(meta['synth'])
    kw['num_blocks'] = tuple(kw['num_blocks'])
    return synth.flexnet_state_dict(seed=meta['seed'], **kw)


def test_fixtures_exist():
    assert len(NAMES) == 5
    metas = {n: load_golden(n)[0] for n in NAMES}
    # the reference's loader claims every checkpoint but the one whose first LBlock has a single block: there it raises KeyError
    assert all((m['claimed_by'], m['loader_error']) == ('FlexNet', '') for n, m in metas.items() if n != ONE_BLOCK_FIRST)
    assert metas[ONE_BLOCK_FIRST]['claimed_by'] == '' and 'pipeline.att.0.t_blocks.2.ffn.key.weight' in metas[ONE_BLOCK_FIRST]['loader_error']
    assert {m['hyper']['upsampler'] for m in metas.values()} == {'ps', 'dys', 'n+c'}
    assert {m['hyper']['dim'] for m in metas.values()} == {16, 32, 48, 64}
    assert all(0.1 <= m['y_absmax'] <= 10 for m in metas.values())


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    claims = [a.id for a in internal_registry.walk() if a.detect(sd)]
    assert claims == ['FlexNet']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, FlexNet)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'FlexNet'
    hy = meta['hyper']
    assert (m.dim, m.in_ch, m.out_ch, list(m.num_blocks), m.hidden_rate, m.channel_norm) == (hy['dim'], hy['inp_channels'], hy['out_channels'], hy['num_blocks'],
                                                                                              hy['hidden_rate'], hy['channel_norm'])  # fmt: skip
    assert (int(m.window_size), m.upsampler, m.scale, m.pad, m.pipeline_type) == (hy['window_size'], hy['upsampler'], hy['scale'], hy['pad'], 'linear')
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
    assert got['window_size'].dtype == torch.uint8 and got['window_size'].dim() == 0
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'pipeline.att.0.t_blocks.0.att.get_v.bias'})
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)))


def test_detection_keys():
    arch = internal_registry.get('FlexNet')
    sd = synth.flexnet_state_dict(dim=16, num_blocks=(1,))
    assert arch.detect(sd)
    for drop in ('short_cut.block.0.weight', 'short_cut.block.0.bias', 'short_cut.block.2.weight', 'short_cut.block.2.bias', 'short_cut.conv11.weight',
                 'short_cut.conv11.bias', 'in_to_feat.weight', 'in_to_feat.bias', 'pipeline.att.0.t_blocks.0.gamma1'):  # fmt: skip
        assert not arch.detect({k: v for k, v in sd.items() if k != drop}), drop
    assert arch.detect({k: v for k, v in sd.items() if k != 'pipeline.att.0.t_blocks.0.gamma2'})  # not a detection key
    assert arch.detect(_meta_checkpoint())  # either of the two gamma1 keys


def test_registry_position():
    """FlexNet is consulted after the ordered walk and after ``late``; both stay what they were.  The registry knows FlexNet by id."""
    ids = list(internal_registry.store)
    meta, _ = load_golden('registry_claims')
    assert 'FlexNet' in meta['order'] and ids == [u for u in meta['order'] if u in ids] and 'FlexNet' not in ids
    assert 'FlexNet' not in internal_registry.late and list(internal_registry.last) == ['FlexNet']
    assert 'FlexNet' in internal_registry and internal_registry.get('FlexNet').id == 'FlexNet'
    assert [a.id for a in internal_registry.walk()] == ids + list(internal_registry.late) + ['FlexNet']
    assert resselt_amd.get('FlexNet') is internal_registry.last['FlexNet']


OTHERS = [
    ('eimn', lambda: synth.eimn_state_dict(num_stages=1)), ('ESRGAN', lambda: synth.rrdbnet_state_dict(nb=1)), ('spanplus', lambda: synth.spanplus_state_dict(blocks=(1,))),
    ('SPAN', lambda: synth.span_state_dict()), ('SwinIR', lambda: synth.swinir_state_dict()), ('Compact', lambda: synth.compact_state_dict(num_conv=2)),
    ('dat', lambda: synth.dat_state_dict()), ('SpanPP', lambda: synth.spanpp_state_dict()), ('HAT', lambda: synth.hat_state_dict()),
    ('RTMoSR', lambda: synth.rtmosr_state_dict()), ('DRCT', lambda: synth.drct_state_dict()), ('PLKSR', lambda: synth.plksr_state_dict()),
    ('PLKSR', lambda: synth.realplksr_state_dict()), ('CuGAN', lambda: synth.cugan_state_dict()), ('MoSR', lambda: synth.mosr_state_dict(n_block=1)),
    ('MoSRv2', lambda: synth.mosrv2_state_dict(n_block=1)), ('RGT', lambda: synth.rgt_state_dict()), ('FDAT', lambda: synth.fdat_state_dict()),
    ('OmniSR', lambda: synth.omnisr_state_dict()), ('ATD', lambda: synth.atd_state_dict()), ('RCAN', lambda: synth.rcan_state_dict(n_resgroups=1, n_resblocks=1)),
    ('GateR', lambda: synth.gater_state_dict(dim=24, num_blocks=(1,) * 7)), ('RHA', lambda: synth.rha_state_dict(dim=16, group_blocks=1, res_blocks=1)),
]  # fmt: skip


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('FlexNet').detect(sd)
    claims = [a.id for a in internal_registry.walk() if a.detect(sd)]
    assert claims and claims[0] == uid and 'FlexNet' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'FlexNet'


def test_every_other_registered_architecture_has_a_checkpoint_above():
    assert {a.id for a in internal_registry.walk()} - {'FlexNet'} == {u for u, _ in OTHERS}


def _meta_checkpoint():
    sd = synth.flexnet_state_dict(dim=16, num_blocks=(1,))
    return {k.replace('pipeline.att.0.', 'pipeline.enc0.0.'): v for k, v in sd.items()}


def test_the_two_refusals():
    with pytest.raises(NotImplementedError, match='meta pipeline is not built'):
        resselt_amd.load_from_state_dict(_meta_checkpoint())
    with pytest.raises(NotImplementedError, match='not built'):
        FlexNet(dim=16, num_blocks=(1, 1, 1, 1), pipeline_type='meta')
    for ws in (4, 16):
        sd = synth.flexnet_state_dict(dim=16, num_blocks=(1,))
        sd['window_size'] = torch.tensor(ws, dtype=torch.uint8)
        with pytest.raises(NotImplementedError, match='get_lepe hardcodes H = W = 8'):
            resselt_amd.load_from_state_dict(sd)


def test_shape_limits():
    with pytest.raises(NotImplementedError, match='multiple of 16 from 16 to 128'):
        FlexNet(dim=24)
    with pytest.raises(NotImplementedError, match='multiple of 16 from 16 to 128'):
        resselt_amd.load_from_state_dict(dict(synth.flexnet_state_dict(dim=144, num_blocks=(1,))))
    with pytest.raises(NotImplementedError, match='input channels'):
        FlexNet(dim=16, inp_channels=9, out_channels=9)
    with pytest.raises(NotImplementedError, match='at least one'):
        FlexNet(dim=16, num_blocks=())
    with pytest.raises(NotImplementedError, match='n\\+c head'):
        FlexNet(dim=16, num_blocks=(1,), scale=5, upsampler='n+c')
    for kw in (dict(dim=128, inp_channels=8, out_channels=8, hidden_rate=1, scale=1), dict(dim=16, upsampler='n+c', scale=1, out_channels=2),
               dict(dim=16, upsampler='n+c', scale=8), dict(dim=48, upsampler='dys', scale=2, inp_channels=1, out_channels=4, channel_norm=True)):  # fmt: skip
        sd = synth.flexnet_state_dict(num_blocks=(1,), **kw)
        m = resselt_amd.load_from_state_dict(dict(sd))  # the limits themselves load
        assert list(m.state_dict()) == list(sd) and (m.dim, m.scale, m.out_ch) == (kw['dim'], kw['scale'], kw.get('out_channels', 3))


def test_hidden_rate_is_read_from_the_first_block():
    """The reference reads t_blocks.2 of the first LBlock and raises KeyError when it has fewer than three blocks; t_blocks.0 gives the same
    value wherever the reference loads."""
    meta, _ = load_golden(ONE_BLOCK_FIRST)
    m = resselt_amd.load_from_state_dict(dict(_sd(meta)))
    assert (list(m.num_blocks), m.hidden_rate, m.hidden) == ([1, 2], 4, 128)
    for nb, rate in (((1,), 1), ((2, 1), 3), ((3,), 2)):
        m = resselt_amd.load_from_state_dict(dict(synth.flexnet_state_dict(dim=16, num_blocks=nb, hidden_rate=rate)))
        assert (m.hidden_rate, m.hidden) == (rate, 16 * rate)


def test_stored_reparam_kernel_has_no_influence():
    sd = synth.flexnet_state_dict(dim=32, num_blocks=(1,), seed=3, channel_norm=True)
    other = dict(sd)
    n = 0
    for k in sd:
        if 'conv5x5_reparam' in k:
            other[k] = torch.full_like(sd[k], 7.0)
            n += 1
    assert n == 2
    b = 'pipeline.att.0.t_blocks.0'
    fa, fb = fold_block(sd, b, 32, True), fold_block(other, b, 32, True)
    assert sorted(fa) == ['kr_w', 'lepe_b', 'lepe_w', 'proj_b', 'proj_w', 'qkv_b', 'qkv_w', 'rn1', 'rn2', 'shift1', 'shift2', 'value_w']
    assert all(torch.equal(fa[k], fb[k]) for k in fa)
    # and the packed kernel is the fold of the training parameters, not the stored weight
    for shift, key in (('shift1', f'{b}.att.omni_shift'), ('shift2', f'{b}.ffn.omni_shift')):
        w = fa[shift].reshape(32, 1, 5, 5)
        assert not torch.allclose(w, sd[f'{key}.conv5x5_reparam.weight'])
        a = sd[f'{key}.alpha'].double()
        assert torch.allclose(w[:, :, 0, 0].double(), a[3] * sd[f'{key}.conv5x5.weight'][:, :, 0, 0].double(), atol=1e-7)  # a corner: the 5x5 branch alone
        centre = a[0] + a[1] * sd[f'{key}.conv1x1.weight'][:, 0, 0, 0].double() + a[2] * sd[f'{key}.conv3x3.weight'][:, 0, 1, 1].double()
        centre = centre + a[3] * sd[f'{key}.conv5x5.weight'][:, 0, 2, 2].double()
        assert torch.equal(w[:, 0, 2, 2], centre.float())  # f64, rounded once
        assert torch.equal(fold_omnishift(other, key), fa[shift])


def test_folds():
    sd = synth.flexnet_state_dict(dim=32, num_blocks=(1,), seed=4, channel_norm=True, hidden_rate=2)
    b = 'pipeline.att.0.t_blocks.0'
    f = fold_block(sd, b, 32, True)
    d = torch.float64
    wq = sd[f'{b}.att.qkv.weight'].to(d)
    assert torch.equal(f['qkv_w'][:32, :, 0, 0], (wq[:32] * 32**-0.5).float()) and torch.equal(f['qkv_w'][32:, :, 0, 0], wq[32:].float())
    assert torch.equal(f['qkv_b'][:32], (sd[f'{b}.att.qkv.bias'][:32].to(d) * 32**-0.5).float()) and torch.equal(f['qkv_b'][32:], sd[f'{b}.att.qkv.bias'][32:])
    g1, g2 = sd[f'{b}.gamma1'].to(d), sd[f'{b}.gamma2'].to(d)
    assert torch.equal(f['proj_w'][:, :, 0, 0], (g1[:, None] * sd[f'{b}.att.proj.weight'].to(d)).float())
    assert torch.equal(f['proj_b'], (g1 * sd[f'{b}.att.proj.bias'].to(d)).float())
    assert torch.equal(f['value_w'][:, :, 0, 0], (g2[:, None] * sd[f'{b}.ffn.value.weight'].to(d) * sd[f'{b}.ffn.key_norm.weight'].to(d)[None, :]).float())
    assert f['kr_w'].shape == (64 + 32, 32, 1, 1) and torch.equal(f['kr_w'][:64, :, 0, 0], sd[f'{b}.ffn.key.weight'])
    assert torch.equal(f['kr_w'][64:, :, 0, 0], sd[f'{b}.ffn.receptance.weight'])
    assert f['lepe_w'].shape == (9, 32) and torch.equal(f['lepe_w'][5], sd[f'{b}.att.get_v.weight'][:, 0, 1, 2])
    plain = fold_block(synth.flexnet_state_dict(dim=32, num_blocks=(1,), seed=4, hidden_rate=2), b, 32, False)
    assert torch.equal(plain['value_w'][:, :, 0, 0], (g2[:, None] * sd[f'{b}.ffn.value.weight'].to(d)).float())
    assert RMS_EPS == torch.finfo(torch.float32).eps == 2.0**-23


def test_macs_against_a_hand_count():
    """dim 32, hidden 128, blocks (1, 2), RGB, n+c x3."""
    m = resselt_amd.load_from_state_dict(dict(_sd(load_golden(ONE_BLOCK_FIRST)[0])))
    block = 2 * 25 * 32 + 3 * 32 * 32 + 2 * 64 * 32 + 9 * 32 + 32 * 32 + (128 + 32) * 32 + 128 * 32  # two shifts, qkv, q k^T and p v, lepe, proj, key | receptance, value
    tail = 9 * 64 * 32 + 9 * 32 * 32 + 64 * 32
    first = 9 * 3 * 32 + 9 * 32 * 32 + 3 * 32 + 9 * 3 * 32  # short_cut and in_to_feat
    head = 9 * 64 * 32 + 9 * 32 * 32 + 9 * (9 * 32 * 32 + 9 * 32 * 3)  # to_img.0, the convolution before the x3 upsampling, two behind it
    want = first + 3 * block + 2 * tail + head
    assert m.macs_per_input_pixel() == want


@pytest.mark.parametrize('ext', ['.pth', '.safetensors'])
def test_load_from_file_round_trip(tmp_path, ext):
    sd = synth.flexnet_state_dict(dim=16, num_blocks=(2,), scale=2, upsampler='n+c', seed=9)
    path = str(tmp_path / f'flexnet{ext}')
    if ext == '.pth':
        torch.save(dict(sd), path)
    else:
        import safetensors.torch

        safetensors.torch.save_file({k: v.contiguous() for k, v in sd.items()}, path)
    m = resselt_amd.load_from_file(path)
    assert isinstance(m, FlexNet) and (m.dim, m.scale, m.upsampler, list(m.num_blocks)) == (16, 2, 'n+c', [2])
    got = m.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], v) for k, v in sd.items())
