"""CPU checks of the LAWFFT loader: detection (each of the reference's 30 keys is needed), its place in the registry (in ``rest``, behind
FIGSR, every older tier unchanged), the inferred hyper-parameters and metadata against what the reference's loader inferred, the parameter
tree against the reference module's state_dict (names, order, shapes, dtypes: the uint8 ``window_size`` and ``upscale.MetaUpsample``
included), that no other architecture's checkpoint and no existing fixture changes owner, every refusal (those of the reference, recorded
in tests/golden/lawfft_probe.npz, and this build's own), the probe's four findings and the file round trips.  On the commit before LAWFFT
every load here raises ``ArchitectureNotFound``."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.lawfft import DETECTION_KEYS
from resselt_amd.archs.lawfft.arch import LAWFFT
from resselt_amd.engine.base import Plan
from resselt_amd.utils import synth
from test_gfisrv2_loader import OTHERS

NAMES = [n for n in golden_names('lawfft_') if n != 'lawfft_probe']
SMALL = dict(dim=32, local=8, n_rblock=1, n_mblock=2, scale=2)
MODES = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample')
ELDERS = OTHERS + [('GFISRV2', lambda: synth.gfisrv2_state_dict(dim=16, n_blocks=1, scale=2)), ('FIGSR', lambda: synth.figsr_state_dict(dim=32, n_blocks=2, scale=2))]


def _sd(meta):
    return synth.lawfft_state_dict(seed=meta['seed'], **meta['synth'])


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert meta['claims'] == ['LAWFFT']  # what the whole reference registry said
    claims = [a.id for a in internal_registry.order() if a.detect(sd)]
    assert claims == ['LAWFFT']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, LAWFFT)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'LAWFFT' and pi.in_channels == pi.out_channels
    hy, kw = meta['hyper'], meta['synth']
    assert (m.in_ch, m.dim, m.scale, m.n_rblock, m.n_mblock, m.head, m.mid_dim) == (hy['in_ch'], hy['dim'], hy['scale'], hy['n_rblock'], hy['n_mblock'], hy['upsampler'], hy['mid_dim'])
    assert hy['window_size'] == 8 and hy['unshuffle_mod'] is False
    # the widths the reference's module computes from the ratios its loader hands over are the ones read from the shapes here
    local = kw.get('local', 15)
    assert hy['split'] == 1 / (hy['dim'] / local) and m.local == int(hy['split'] * hy['dim']) == local and m.glob == hy['dim'] - local
    assert m.fsas == int(m.glob * hy['t_mid_factor']) == sd['body.0.residual.0.token_mix.1.att.norm.weight'].shape[0]
    assert 3 * m.fsas == int(m.glob * 3 * hy['t_mid_factor']) == sd['body.0.residual.0.token_mix.1.att.to_hidden.bias'].shape[0]
    assert m.hidden == int(hy['dim'] * hy['mlp_factor']) == sd['body.0.residual.0.channel_mix1.1.project_out.weight'].shape[1]
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'fp16') and m.global_statistics
    assert m.macs_per_input_pixel() > 0


@pytest.mark.parametrize('name', NAMES)
def test_parameter_tree_equals_the_reference_modules(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert list(sd) == list(meta['state_dict']) and {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert list(got) == list(meta['state_dict'])  # names and registration order of the reference module
    assert all(list(got[k].shape) == v for k, v in meta['state_dict'].items())
    assert {k: str(v.dtype) for k, v in got.items() if v.dtype != torch.float32} == meta['dtypes'] == {'window_size': 'torch.uint8', 'upscale.MetaUpsample': 'torch.uint8'}
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    hy = meta['hyper']
    assert [int(v) for v in got['upscale.MetaUpsample']] == [2, MODES.index(hy['upsampler']), hy['scale'], hy['dim'], hy['in_ch'], hy['mid_dim'], 4]
    assert list(got)[0] == 'window_size' and int(got['window_size']) == 8
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'body.0.residual.0.token_mix.1.att.norm.weight'})


def test_each_detection_key_is_needed():
    arch = internal_registry.get('LAWFFT')
    sd = synth.lawfft_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 30 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        less = {k: v for k, v in sd.items() if k != drop}
        assert not arch.detect(less), drop
        with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
            resselt_amd.load_from_state_dict(less)
    assert arch.detect({k: v for k, v in sd.items() if k not in ('window_size', 'upscale.MetaUpsample')})  # not detection keys


def test_registry_position():
    """LAWFFT sits in ``rest`` behind FIGSR, and none of the older tiers and iterators knows it."""
    r = internal_registry
    assert all('LAWFFT' not in t for t in (r.store, r.late, r.last, r.after, r.tail)) and 'LAWFFT' in r.rest
    rest = list(r.rest)
    assert rest == ['GFISRV2', 'FIGSR', 'LAWFFT']
    every = [a.id for a in r.every()]
    order = [a.id for a in r.order()]
    assert 'LAWFFT' not in every and 'LAWFFT' not in [a.id for a in r] and 'LAWFFT' not in [a.id for a in r.walk()] and 'LAWFFT' not in [a.id for a in r.consulted()]
    assert order[: len(every)] == every and order[len(every) :] == rest and len(r) == len(r.store) + len(r.late)
    assert list(r.late) == ['RHA'] and list(r.last) == ['FlexNet'] and list(r.after) == ['MoESR'] and list(r.tail) == ['SMoSR']
    assert 'LAWFFT' in r and r.get('LAWFFT').id == 'LAWFFT' and resselt_amd.get('LAWFFT') is r.rest['LAWFFT']
    meta, _ = load_golden('registry_claims')
    assert 'LAWFFT' in meta['order']


@pytest.mark.parametrize('uid,make', ELDERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(ELDERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('LAWFFT').detect(sd)
    claims = [a.id for a in internal_registry.order() if a.detect(sd)]
    assert claims and claims[0] == uid and 'LAWFFT' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'LAWFFT'


def test_no_existing_fixture_of_any_family_is_claimed():
    """Every golden fixture that records a state dict's names: none of them has LAWFFT's detection keys."""
    arch, seen = internal_registry.get('LAWFFT'), 0
    for name in golden_names(''):
        meta, _ = load_golden(name)
        keys = meta.get('state_dict') if isinstance(meta, dict) else None
        if not isinstance(keys, (dict, list)) or name.startswith('lawfft_'):
            continue
        seen += 1
        assert not arch.detect({k: None for k in keys}), name
    assert seen >= 50


def test_every_architecture_consulted_before_it_has_a_checkpoint_above():
    order = [a.id for a in internal_registry.order()]
    assert set(order[: order.index('LAWFFT')]) <= {u for u, _ in ELDERS}


def test_the_probes_four_findings():
    """tests/golden/lawfft_probe.npz: where the reference refuses, and what this build does there."""
    meta, _ = load_golden('lawfft_probe')
    seed = meta['seed']
    # 1. the reflect pad on the bottom and right: p = (8 - side % 8) % 8 pixels need more than p of them
    probe = {tuple(p['size']): p['raises'] for p in meta['probe']}
    assert probe == {(4, 8): 'RuntimeError', (8, 4): 'RuntimeError', (3, 9): 'RuntimeError', (5, 8): None, (8, 5): None, (8, 8): None, (9, 12): None}
    m = resselt_amd.load_from_state_dict(dict(_sd(meta)))
    for (h, w), raises in probe.items():
        if raises is not None:
            with pytest.raises(RuntimeError, match='Padding size should be less'):  # before anything is allocated or launched
                m._build_plan(Plan('cpu'), {}, (1, 3, h, w), torch.float32, m.products)
    for side in range(1, 5):
        with pytest.raises(RuntimeError, match='Padding size should be less'):
            m._build_plan(Plan('cpu'), {}, (1, 3, side, 16), torch.float32, m.products)
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m._build_plan(Plan('cpu'), {}, (1, 1, 9, 9), torch.float32, m.products)
    # 2. unshuffle_mod: nobody in the reference detects the checkpoint (in_to_dim.weight is a detection key), and handed to the loader
    # directly the module is built with the plain stem (MetaUpsample stores scale 4) and cannot take the state dict
    un = meta['unshuffle']
    assert un['claims'] == [] and un['registry']['raises'] == 'ArchitectureNotFound'
    assert un['loader']['raises'] == 'RuntimeError' and 'loading state_dict' in un['loader']['message']
    sd = synth.lawfft_state_dict(seed=seed, **un['synth'])
    assert 'in_to_dim.1.weight' in sd and 'in_to_dim.weight' not in sd and not internal_registry.get('LAWFFT').detect(sd)
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        resselt_amd.load_from_state_dict(dict(sd))
    with pytest.raises(NotImplementedError, match='unshuffle_mod'):
        internal_registry.get('LAWFFT').load(dict(sd))
    # 3. a (dim, local) pair whose float split lands on local - 1: the reference's own module rejects the state dict, the engine loads it
    fs = meta['float_split']
    d, lo = fs['synth']['dim'], fs['synth']['local']
    assert [d, lo] == fs['pairs'][0] and fs['count'] > 0 and int((1 / (d / lo)) * d) == fs['int_split_dim'] == lo - 1
    assert fs['raises'] == 'RuntimeError' and 'loading state_dict' in fs['message']
    assert all(int((1 / (a / b)) * a) != b for a, b in fs['pairs'])
    sd = synth.lawfft_state_dict(seed=seed, **fs['synth'])
    mf = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(mf, LAWFFT) and (mf.dim, mf.local, mf.glob) == (d, lo, d - lo)
    assert all(torch.equal(mf.state_dict()[k], v) for k, v in sd.items())
    # 4. n_mblock = 1: the reference's loader reads block 1 and raises KeyError; refused by name here
    one = meta['one_block']
    assert one['raises'] == 'KeyError' and 'body.0.residual.1' in one['message']
    with pytest.raises(NotImplementedError, match='at least two MetaBlocks'):
        resselt_amd.load_from_state_dict(dict(synth.lawfft_state_dict(seed=seed, **one['synth'])))


def test_the_refusals_of_this_build():
    load = lambda **kw: resselt_amd.load_from_state_dict(dict(synth.lawfft_state_dict(**dict(SMALL, **kw))))  # noqa: E731
    with pytest.raises(NotImplementedError, match='window_size 4 is not built'):
        load(window_size=4)
    with pytest.raises(NotImplementedError, match='window_size 16 is not built'):
        LAWFFT(window_size=16)
    with pytest.raises(NotImplementedError, match='3 x the FSAS width'):
        load(to_hidden_rows=71)  # 71 rows beside a norm of 24: q, k and v are no equal chunks
    with pytest.raises(NotImplementedError, match='3 x the FSAS width'):
        LAWFFT(dim=60, split=0.25, t_mid_factor=0.5)  # int(45 * 0.5) = 22, int(45 * 3 * 0.5) = 67
    both = synth.lawfft_state_dict(**SMALL)
    both['in_to_dim.1.weight'] = torch.zeros(32, 12, 3, 3)
    with pytest.raises(NotImplementedError, match='unshuffle_mod'):
        resselt_amd.load_from_state_dict(dict(both))
    with pytest.raises(NotImplementedError, match='dim must be in 2..128'):
        load(dim=136, local=34)
    with pytest.raises(NotImplementedError, match='FSAS width'):
        load(dim=128, local=8, t_mid_factor=1.25)  # 150
    with pytest.raises(NotImplementedError, match='at least two MetaBlocks'):
        load(n_mblock=1)
    with pytest.raises(NotImplementedError, match='local and the global width'):
        LAWFFT(dim=32, split=0.0)
    with pytest.raises(NotImplementedError, match='mid_dim to be a multiple of 8'):
        load(upsampler='pixelshuffle', mid_dim=20)
    with pytest.raises(NotImplementedError, match='mid_dim to be a multiple of 8'):
        load(upsampler='dysample', mid_dim=20)
    with pytest.raises(ValueError, match='invalid Upsample'):
        LAWFFT(upsampler='bicubic')
    with pytest.raises(ValueError, match='scale 5 is not supported'):
        LAWFFT(scale=5, upsampler='pixelshuffle')
    for kw in (dict(dim=128, local=32), dict(scale=8), dict(scale=8, upsampler='pixelshuffle', mid_dim=16), dict(scale=8, upsampler='nearest+conv'), dict(mlp_factor=0.05),
               dict(dim=60, local=15, upsampler='dysample', mid_dim=60), dict(n_rblock=3, n_mblock=3), dict(dim=30, local=7)):
        assert isinstance(load(**kw), LAWFFT), kw


def test_file_round_trips(tmp_path):
    from safetensors.torch import save_file

    sd = synth.lawfft_state_dict(**SMALL, upsampler='dysample', mid_dim=24, seed=9)
    torch.save(dict(sd), tmp_path / 'm.pth')
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'm.safetensors'))
    for name in ('m.pth', 'm.safetensors'):
        m = resselt_amd.load_from_file(str(tmp_path / name))
        assert isinstance(m, LAWFFT) and m.parameters_info.name == 'LAWFFT'
        got = m.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], v) and got[k].dtype == v.dtype for k, v in sd.items())
