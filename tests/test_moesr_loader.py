"""CPU checks of the MoESR loader: detection (each of the reference's sixteen keys is needed), its place behind the registry's walk in the
open-ended ``after`` tier, the inferred hyper-parameters and metadata against what the reference's loader inferred, the parameter tree
against the reference module's state_dict (names, order, shapes, dtypes), that no other architecture's checkpoint changes owner, the three
refusals, ``hidden`` read from the shapes, the MAC count and the file round trip."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.moesr import DETECTION_KEYS
from resselt_amd.archs.moesr.arch import MoESR
from resselt_amd.factory import Architecture, KeyCondition
from resselt_amd.registry import Registry
from resselt_amd.utils import synth

NAMES = golden_names('moesr_')
SMALL = dict(dim=16, n_blocks=1, n_block=1, scale=2)


def _sd(meta):
    return synth.moesr_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures_exist():
    assert len(NAMES) == 7
    metas = {n: load_golden(n)[0] for n in NAMES}
    assert all(m['claimed_by'] == 'MoESR' and m['claims'] == ['MoESR'] for m in metas.values())  # in the reference's registry too
    assert {m['hyper']['upsampler'] for m in metas.values()} == {'conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample'}
    assert {m['hyper']['dim'] for m in metas.values()} == {32, 40, 48, 64}
    assert all(0.1 <= m['y_absmax'] <= 10 for m in metas.values())
    full = metas['moesr_x4_full_d64_g9b4_9x11']['hyper']
    assert (full['n_blocks'], full['n_block']) == (9, 4)  # the default depth: 9 * (4 + 3) = 63 gated blocks


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    claims = [a.id for a in internal_registry.consulted() if a.detect(sd)]
    assert claims == ['MoESR']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, MoESR)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'MoESR'
    hy = meta['hyper']
    assert (m.in_ch, m.out_ch, m.scale, m.n_blocks, m.n_block, m.dim, m.head, m.upsample_dim) == (
        hy['in_ch'], hy['out_ch'], hy['scale'], hy['n_blocks'], hy['n_block'], hy['dim'], hy['upsampler'], hy['upsample_dim'])  # fmt: skip
    assert (m.expansion_factor, m.expansion_msg) == (hy['expansion_factor'], hy['expansion_msg'])  # the same expression, the same floats
    assert m.hidden == sd['blocks.0.blocks.0.fc2.weight'].shape[1] and m.hidden_msg == sd['blocks.0.msg.gated.0.fc2.weight'].shape[1]
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'fp16')


@pytest.mark.parametrize('name', NAMES)
def test_parameter_tree_equals_the_reference_modules(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert list(sd) == list(meta['state_dict']) and {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert list(got) == list(meta['state_dict'])  # names and registration order of the reference module
    assert all(list(got[k].shape) == v for k, v in meta['state_dict'].items())
    assert {k: str(v.dtype) for k, v in got.items() if v.dtype != torch.float32} == meta['dtypes'] == {'upscale.MetaUpsample': 'torch.uint8'}
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'blocks.0.msg.up.0.bias'})
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)))


def test_each_of_the_sixteen_detection_keys_is_needed():
    arch = internal_registry.get('MoESR')
    sd = synth.moesr_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 16 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        less = {k: v for k, v in sd.items() if k != drop}
        assert not arch.detect(less), drop
        with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
            resselt_amd.load_from_state_dict(less)
    assert arch.detect({k: v for k, v in sd.items() if k != 'blocks.0.msg.down.0.weight'})  # not a detection key


def test_registry_position():
    """MoESR is consulted after everything ``walk()`` yields; ``store``, ``late``, ``last``, iteration, ``len()`` and ``walk()`` do not know it."""
    r = internal_registry
    assert list(r.after) == ['MoESR'] and all('MoESR' not in t for t in (r.store, r.late, r.last))
    walked = [a.id for a in r.walk()]
    assert 'MoESR' not in walked and 'MoESR' not in [a.id for a in r] and len(r) == len(r.store) + len(r.late)
    assert [a.id for a in r.consulted()] == walked + ['MoESR']
    assert 'MoESR' in r and r.get('MoESR').id == 'MoESR' and resselt_amd.get('MoESR') is r.after['MoESR']
    with pytest.raises(KeyError):
        r.get('NoSuchArch')
    meta, _ = load_golden('registry_claims')
    assert 'MoESR' in meta['order']  # the reference walks it inside its order; here its place cannot matter (the tests below)


def test_the_after_tier_is_general():
    """Any number of entries, in insertion order; re-registering replaces in place; an id the walk already holds stays where it is."""
    class Stub(Architecture):
        def load(self, state_dict):
            raise AssertionError('never built')

    mk = lambda uid: Stub(uid=uid, detect=KeyCondition.has_all(uid))  # noqa: E731
    r = Registry()
    a, b, c, s = mk('A'), mk('B'), mk('C'), mk('S')
    r.add(s)
    r.add(a, after=True)
    r.add(b, after=True)
    r.add(c, late=True)
    assert list(r.after) == ['A', 'B'] and [x.id for x in r.consulted()] == ['S', 'C', 'A', 'B'] and [x.id for x in r.walk()] == ['S', 'C']
    assert len(r) == 2 and [x.id for x in r] == ['S', 'C'] and 'B' in r and r.get('B') is b
    a2 = mk('A')
    r.add(a2, after=True)
    assert list(r.after) == ['A', 'B'] and r.get('A') is a2
    r.add(mk('S'), after=True)  # already in the walk: replaced there
    assert 'S' not in r.after and list(r.store) == ['S']
    r.add(mk('B'))  # moved into the walk on request
    assert list(r.after) == ['A'] and list(r.store) == ['S', 'B']


OTHERS = [
    ('eimn', lambda: synth.eimn_state_dict(num_stages=1)), ('ESRGAN', lambda: synth.rrdbnet_state_dict(nb=1)), ('spanplus', lambda: synth.spanplus_state_dict(blocks=(1,))),
    ('SPAN', lambda: synth.span_state_dict()), ('SwinIR', lambda: synth.swinir_state_dict()), ('Compact', lambda: synth.compact_state_dict(num_conv=2)),
    ('dat', lambda: synth.dat_state_dict()), ('SpanPP', lambda: synth.spanpp_state_dict()), ('HAT', lambda: synth.hat_state_dict()),
    ('RTMoSR', lambda: synth.rtmosr_state_dict()), ('DRCT', lambda: synth.drct_state_dict()), ('PLKSR', lambda: synth.plksr_state_dict()),
    ('PLKSR', lambda: synth.realplksr_state_dict()), ('CuGAN', lambda: synth.cugan_state_dict()), ('MoSR', lambda: synth.mosr_state_dict(n_block=1)),
    ('MoSRv2', lambda: synth.mosrv2_state_dict(n_block=1)), ('MoSRv2', lambda: synth.mosrv2_state_dict(n_block=1, unshuffle_mod=False, upsampler='dysample')),
    ('RGT', lambda: synth.rgt_state_dict()), ('FDAT', lambda: synth.fdat_state_dict()),
    ('OmniSR', lambda: synth.omnisr_state_dict()), ('ATD', lambda: synth.atd_state_dict()), ('RCAN', lambda: synth.rcan_state_dict(n_resgroups=1, n_resblocks=1)),
    ('GateR', lambda: synth.gater_state_dict(dim=24, num_blocks=(1,) * 7)), ('RHA', lambda: synth.rha_state_dict(dim=16, group_blocks=1, res_blocks=1)),
    ('FlexNet', lambda: synth.flexnet_state_dict(dim=16, num_blocks=(1,))),
]  # fmt: skip


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('MoESR').detect(sd)
    claims = [a.id for a in internal_registry.consulted() if a.detect(sd)]
    assert claims and claims[0] == uid and 'MoESR' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'MoESR'


def test_every_other_registered_architecture_has_a_checkpoint_above():
    assert {a.id for a in internal_registry.consulted()} - {'MoESR'} == {u for u, _ in OTHERS}


def test_the_three_refusals():
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        resselt_amd.load_from_state_dict(dict(synth.moesr_state_dict(**dict(SMALL, dim=36))))
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        MoESR(dim=36)
    with pytest.raises(NotImplementedError, match='dim above 128 is not built'):
        resselt_amd.load_from_state_dict(dict(synth.moesr_state_dict(**dict(SMALL, dim=136))))
    with pytest.raises(NotImplementedError, match='hidden must be at least dim'):
        resselt_amd.load_from_state_dict(dict(synth.moesr_state_dict(**dict(SMALL, expansion_factor=0.75))))
    with pytest.raises(NotImplementedError, match='hidden must be at least dim'):
        MoESR(dim=16, expansion_msg=0.5)
    m = resselt_amd.load_from_state_dict(dict(synth.moesr_state_dict(**dict(SMALL, dim=128, expansion_factor=1.0, expansion_msg=1.0))))  # the limits load
    assert (m.dim, m.hidden, m.hidden_msg) == (128, 128, 128)


def test_hidden_is_read_from_the_shapes():
    """A checkpoint whose hidden width the inferred float ratio does not reproduce: hidden 61 of dim 56, int(((122 / 56) / 2) * 56) == 60."""
    assert int(((122 / 56) / 2) * 56) == 60
    sd = synth.moesr_state_dict(**dict(SMALL, dim=56))
    gen = torch.Generator().manual_seed(0)
    for k in list(sd):
        if k.startswith('blocks.0.blocks.') and (k.endswith('.fc1.weight') or k.endswith('.fc1.bias')):
            sd[k] = torch.randn((122, *sd[k].shape[1:]), generator=gen) * 0.05
        elif k.startswith('blocks.0.blocks.') and k.endswith('.fc2.weight'):
            sd[k] = torch.randn((56, 61, 3, 3), generator=gen) * 0.05
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert m.hidden == 61 and m.hidden_msg == 84 and m.expansion_factor == (122 / 56) / 2
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())


def test_macs_against_a_hand_count():
    """dim 32, hidden 85 / 48, two groups of one block, RGB, x2 pixelshuffledirect."""
    m = resselt_amd.load_from_state_dict(dict(_sd(load_golden('moesr_x2_psd_d32_g2b1_9x11')[0])))
    blk = lambda h: 9 * 32 * 2 * h + 31 * 4 + 9 * h * 32  # noqa: E731  (fc1, the three depthwise branches of 4 channels, fc2)
    msg = 9 * 32 * 8 + (3 * blk(48) + 9 * 32 * 128) // 4  # down at full resolution; three blocks and up on a quarter of the pixels
    assert m.macs_per_input_pixel() == 9 * 3 * 32 + 2 * (blk(85) + msg) + 9 * 32 * 12


@pytest.mark.parametrize('ext', ['.pth', '.safetensors'])
def test_load_from_file_round_trip(tmp_path, ext):
    sd = synth.moesr_state_dict(**dict(SMALL, upsampler='nearest+conv'), seed=9)
    path = str(tmp_path / f'moesr{ext}')
    if ext == '.pth':
        torch.save(dict(sd), path)
    else:
        import safetensors.torch

        safetensors.torch.save_file({k: v.contiguous() for k, v in sd.items()}, path)
    m = resselt_amd.load_from_file(path)
    assert isinstance(m, MoESR) and (m.dim, m.scale, m.head, m.n_blocks, m.n_block) == (16, 2, 'nearest+conv', 1, 1)
    got = m.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], v) for k, v in sd.items())
