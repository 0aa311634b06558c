"""CPU checks of the FIGSR loader: detection (each of the reference's 57 keys is needed), its place in the registry (in ``rest``, behind
GFISRv2, every older tier unchanged), the inferred hyper-parameters and metadata against what the reference's loader inferred, the
parameter tree against the reference module's state_dict (names, order, shapes, dtypes), that no other architecture's checkpoint and no
existing fixture changes owner, every refusal (those of the reference, recorded in tests/golden/figsr_probe.npz, and this build's own)
and the file round trips.  On the commit before FIGSR every load here raises ``ArchitectureNotFound``."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.figsr import DETECTION_KEYS
from resselt_amd.archs.figsr.arch import FIGSR
from resselt_amd.engine.base import Plan
from resselt_amd.utils import synth
from test_gfisrv2_loader import OTHERS

NAMES = [n for n in golden_names('figsr_') if n != 'figsr_probe']
SMALL = dict(dim=32, n_blocks=2, scale=2)
MODES = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up')


def _sd(meta):
    return synth.figsr_state_dict(seed=meta['seed'], **meta['synth'])


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert meta['claims'] == ['FIGSR']  # what the whole reference registry said
    claims = [a.id for a in internal_registry.order() if a.detect(sd)]
    assert claims == ['FIGSR']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, FIGSR)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'FIGSR'
    hy = meta['hyper']
    assert (m.in_ch, m.out_ch, m.dim, m.scale, m.n_block, m.head, m.mid_dim, m.gc, m.ksq, m.kband) == (
        hy['in_nc'], hy['out_nc'], hy['dim'], hy['scale'], hy['n_blocks'], hy['upsampler'], hy['mid_dim'], hy['gc'], hy['square_kernel_size'], hy['band_kernel_size'])  # fmt: skip
    fc1 = sd['gfisr_body_half.0.fc1.weight'].shape[0]
    assert hy['expansion_ratio'] == fc1 / 2 / hy['dim'] and m.hidden == int(hy['expansion_ratio'] * hy['dim']) // 8 * 8 == fc1 // 2
    assert m.halves == (hy['n_blocks'] // 2, hy['n_blocks'] - hy['n_blocks'] // 2) and m.cf == hy['dim'] - 3 * hy['gc']
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'fp16') and m.global_statistics and m.rms_norm
    assert m.macs_per_input_pixel() > 0


def test_hidden_widths_of_the_reference():
    """The ``hidden`` the reference computes for the configurations its loader round-trips."""
    for kw, hidden in ((dict(), 128), (dict(dim=32), 80), (dict(dim=40), 104), (dict(dim=64), 168), (dict(dim=32, expansion_ratio=2.0), 64)):
        sd = synth.figsr_state_dict(n_blocks=2, **kw)
        assert sd['gfisr_body_half.0.fc2.weight'].shape[1] == hidden
        assert resselt_amd.load_from_state_dict(dict(sd)).hidden == hidden


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
    hy = meta['hyper']
    assert [int(v) for v in got['upscale.MetaUpsample']] == [3, MODES.index(hy['upsampler']), hy['scale'], hy['dim'], hy['out_nc'], hy['mid_dim'], 4]
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'gfisr_body_half.0.conv.fu.rn.scale'})


def test_a_fresh_module_has_the_references_initial_normalisation():
    m = FIGSR(**SMALL)
    sd = m.state_dict()
    assert torch.equal(sd['shift'], torch.full((1, 3, 1, 1), 0.5)) and torch.equal(sd['scale_norm'], torch.ones(1, 3, 1, 1) / 6)
    assert torch.equal(sd['gfisr_body_half.0.norm.eps'], torch.ones(1) * 1e-6) and torch.equal(sd['gfisr_body_half.0.norm.rms'], torch.ones(1) * 32**-0.5)
    assert torch.equal(sd['gfisr_body_half_2.0.conv.fu.rn.rms'], torch.ones(1) * 16**-0.5) and torch.equal(sd['gfisr_body_half.0.conv.fu.post_norm.scale'], torch.ones(8))


def test_each_detection_key_is_needed():
    arch = internal_registry.get('FIGSR')
    sd = synth.figsr_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 57 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        less = {k: v for k, v in sd.items() if k != drop}
        assert not arch.detect(less), drop
        with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
            resselt_amd.load_from_state_dict(less)
    assert arch.detect({k: v for k, v in sd.items() if k != 'shift'})  # not a detection key


def test_registry_position():
    """FIGSR sits in ``rest`` behind GFISRv2, and none of the older tiers and iterators knows it."""
    r = internal_registry
    assert all('FIGSR' not in t for t in (r.store, r.late, r.last, r.after, r.tail)) and 'FIGSR' in r.rest
    rest = list(r.rest)
    assert rest.index('FIGSR') > rest.index('GFISRV2') and rest[:2] == ['GFISRV2', 'FIGSR']
    every = [a.id for a in r.every()]
    order = [a.id for a in r.order()]
    assert 'FIGSR' not in every and 'FIGSR' not in [a.id for a in r] and 'FIGSR' not in [a.id for a in r.walk()] and 'FIGSR' not in [a.id for a in r.consulted()]
    assert order[: len(every)] == every and order[len(every) :] == rest and len(r) == len(r.store) + len(r.late)
    assert list(r.late) == ['RHA'] and list(r.last) == ['FlexNet'] and list(r.after) == ['MoESR'] and list(r.tail) == ['SMoSR']
    assert 'FIGSR' in r and r.get('FIGSR').id == 'FIGSR' and resselt_amd.get('FIGSR') is r.rest['FIGSR']
    meta, _ = load_golden('registry_claims')
    assert 'FIGSR' in meta['order']


@pytest.mark.parametrize('uid,make', OTHERS + [('GFISRV2', lambda: synth.gfisrv2_state_dict(dim=16, n_blocks=1, scale=2))],
                         ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)] + ['GFISRV2'])  # fmt: skip
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('FIGSR').detect(sd)
    claims = [a.id for a in internal_registry.order() if a.detect(sd)]
    assert claims and claims[0] == uid and 'FIGSR' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'FIGSR'


def test_no_existing_fixture_of_any_family_is_claimed():
    """Every golden fixture that records a state dict's names: none of them has FIGSR's detection keys."""
    arch, seen = internal_registry.get('FIGSR'), 0
    for name in golden_names(''):
        meta, _ = load_golden(name)
        keys = meta.get('state_dict') if isinstance(meta, dict) else None
        if not isinstance(keys, (dict, list)) or name.startswith('figsr_'):
            continue
        seen += 1
        assert not arch.detect({k: None for k in keys}), name
    assert seen >= 50


def test_every_architecture_consulted_before_it_has_a_checkpoint_above():
    order = [a.id for a in internal_registry.order()]
    assert set(order[: order.index('FIGSR')]) <= {u for u, _ in OTHERS} | {'GFISRV2'}


def test_the_references_own_refusals():
    """tests/golden/figsr_probe.npz: where the reference refuses, this build refuses the same way."""
    meta, _ = load_golden('figsr_probe')
    seed = meta['seed']
    # one block: an empty first half, no detection keys, nobody claims it
    one = meta['one_block']
    assert one['raises'] == 'ArchitectureNotFound'
    sd = synth.figsr_state_dict(seed=seed, **one['synth'])
    assert not internal_registry.get('FIGSR').detect(sd)
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        resselt_amd.load_from_state_dict(dict(sd))
    with pytest.raises(NotImplementedError, match='at least two blocks'):
        FIGSR(**one['synth'])
    # one channel: the reference builds and loads it and raises in forward (shift broadcasts the image to 3 channels); refused at load here
    gray = meta['gray']
    assert gray['load']['raises'] is None and gray['forward']['raises'] == 'RuntimeError' and gray['metadata']['in_channels'] == 1
    with pytest.raises(NotImplementedError, match='3 input and 3 output channels'):
        resselt_amd.load_from_state_dict(dict(synth.figsr_state_dict(seed=seed, **gray['synth'])))
    # halves that are not the (n // 2, n - n // 2) split: the reference module cannot take the state dict
    un = meta['uneven_halves']
    assert un['raises'] == 'RuntimeError' and 'loading state_dict' in un['message']
    kw = dict(un['synth'], halves=tuple(un['synth']['halves']))
    with pytest.raises(NotImplementedError, match='halves must be the'):
        resselt_amd.load_from_state_dict(dict(synth.figsr_state_dict(seed=seed, **kw)))
    # the reflect pad: 4 + H % 2 < H
    probe = {tuple(p['size']): p['raises'] for p in meta['probe']}
    assert probe == {(5, 5): 'RuntimeError', (5, 6): 'RuntimeError', (4, 8): 'RuntimeError', (6, 6): None, (8, 9): None, (12, 7): None}
    m = resselt_amd.load_from_state_dict(dict(synth.figsr_state_dict(seed=seed, **meta['synth'])))
    for (h, w), raises in probe.items():
        if raises is not None:
            with pytest.raises(RuntimeError, match='Padding size should be less'):  # before anything is allocated or launched
                m._build_plan(Plan('cpu'), {}, (1, 3, h, w), torch.float32, m.products)
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m._build_plan(Plan('cpu'), {}, (1, 1, 9, 9), torch.float32, m.products)


def test_the_refusals_of_this_build():
    load = lambda **kw: resselt_amd.load_from_state_dict(dict(synth.figsr_state_dict(**dict(SMALL, **kw))))  # noqa: E731
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        load(dim=36)
    with pytest.raises(NotImplementedError, match='dim - 3 gc must be in 8..128'):
        FIGSR(dim=24, n_blocks=2)  # cf = 0: nothing for the FourierUnit (the reference cannot build it either)
    with pytest.raises(NotImplementedError, match='dim - 3 gc must be in 8..128'):
        load(dim=168, expansion_ratio=1.0)  # cf = 144
    with pytest.raises(NotImplementedError, match='gc must be 8 or 16'):
        load(gc=4, square_kernel_size=7, band_kernel_size=11)  # (the reference loads it)
    with pytest.raises(NotImplementedError, match='gc must be 8 or 16'):
        load(dim=96, gc=24)
    with pytest.raises(NotImplementedError, match='square kernel size must be odd, 3..31'):
        load(square_kernel_size=33)
    with pytest.raises(NotImplementedError, match='band kernel size must be odd, 3..31'):
        load(band_kernel_size=33)
    with pytest.raises(NotImplementedError, match='band kernel size must be odd, 3..31'):
        FIGSR(**SMALL, band_kernel_size=12)
    with pytest.raises(NotImplementedError, match='square kernel size must be odd, 3..31'):
        FIGSR(**SMALL, square_kernel_size=1)
    with pytest.raises(NotImplementedError, match='at least dim'):
        load(expansion_ratio=0.75)
    for head in ('transpose+conv', 'lda', 'pa_up'):
        with pytest.raises(NotImplementedError, match='head is not built'):
            FIGSR(**SMALL, upsampler=head)
        assert isinstance(FIGSR(dim=32, n_blocks=2, scale=1, upsampler=head), FIGSR)  # at scale 1 every mode is the one convolution
    with pytest.raises(NotImplementedError, match='hidden widths must be multiples of 8'):
        load(upsampler='pixelshuffle', mid_dim=20)
    with pytest.raises(ValueError, match='invalid Upsample'):
        FIGSR(upsampler='bicubic')
    assert isinstance(load(dim=152, expansion_ratio=1.0), FIGSR) and isinstance(load(band_kernel_size=31, square_kernel_size=3), FIGSR)


def test_file_round_trips(tmp_path):
    from safetensors.torch import save_file

    sd = synth.figsr_state_dict(**SMALL, upsampler='dysample', mid_dim=24, seed=9)
    torch.save(dict(sd), tmp_path / 'm.pth')
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'm.safetensors'))
    for name in ('m.pth', 'm.safetensors'):
        m = resselt_amd.load_from_file(str(tmp_path / name))
        assert isinstance(m, FIGSR) and m.parameters_info.name == 'FIGSR'
        got = m.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], v) and got[k].dtype == v.dtype for k, v in sd.items())
