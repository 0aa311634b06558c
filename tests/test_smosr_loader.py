"""CPU checks of the SMoSR loader: detection (each of the reference's keys is needed), its place in the registry's ``tail`` tier, the
inferred hyper-parameters and metadata against what the reference's loader inferred, the parameter tree against the reference module's
state_dict (names, order, shapes, dtypes), that no other architecture's checkpoint changes owner, the refusals, the size limit of the
reflect pad and the file round trips.  On the commit before SMoSR every load here raises ``ArchitectureNotFound``."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.smosr import DETECTION_KEYS
from resselt_amd.archs.smosr.arch import SMoSR
from resselt_amd.engine.base import Plan
from resselt_amd.utils import synth

NAMES = golden_names('smosr_')
SMALL = dict(dim=16, n_mb=1)


def _sd(meta):
    return synth.smosr_state_dict(seed=meta['seed'], **meta['synth'])


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    claims = [a.id for a in internal_registry.every() if a.detect(sd)]
    assert claims == ['SMoSR']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, SMoSR)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'SMoSR'
    hy = meta['hyper']
    assert (m.in_ch, m.out_ch, m.dim, m.scale, int(m.rep), m.n_mb, m.head, m.mid_dim, m.d_kernel) == (
        hy['in_ch'], hy['out_ch'], hy['dim'], hy['scale'], hy['rep'], hy['n_mb'], hy['upsampler'], hy['upsampler_mid_dim'], hy['d_kernel'])  # fmt: skip
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'fp16')
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
    assert {k: str(v.dtype) for k, v in got.items() if v.dtype != torch.float32} == meta['dtypes'] == {'upsampler.MetaUpsample': 'torch.uint8'}
    assert any(k.endswith('.d_diag') for k in got) and any(k.endswith('.mul') for k in got) and any('.eval_conv.' in k for k in got)
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    # every byte of the buffer, the in_dim slot the loader does not read included, is what a freshly constructed reference module holds
    assert [int(v) for v in got['upsampler.MetaUpsample']] == meta['meta_upsample']
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'end_block.1.eval_conv.bias' and k != 'end_block.1.conv.1.d_diag'} | {'x': torch.zeros(1)})
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.endswith('.mul')})


def test_each_detection_key_is_needed():
    arch = internal_registry.get('SMoSR')
    sd = synth.smosr_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 31 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        less = {k: v for k, v in sd.items() if k != drop}
        assert not arch.detect(less), drop
        with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
            resselt_amd.load_from_state_dict(less)
    assert arch.detect({k: v for k, v in sd.items() if k != 'blocks_1.0.body.0.W'})  # not a detection key


def test_registry_position():
    """SMoSR sits in ``tail``, consulted last; ``store``, ``late``, ``last``, ``after``, iteration, ``len()``, ``walk()`` and
    ``consulted()`` do not know it."""
    r = internal_registry
    assert list(r.tail) == ['SMoSR'] and all('SMoSR' not in t for t in (r.store, r.late, r.last, r.after))
    walked = [a.id for a in r.walk()]
    assert 'SMoSR' not in walked and 'SMoSR' not in [a.id for a in r] and len(r) == len(r.store) + len(r.late)
    consulted = [a.id for a in r.consulted()]
    assert consulted == walked + list(r.after) and 'SMoSR' not in consulted
    assert [a.id for a in r.every()] == consulted + ['SMoSR']
    assert 'SMoSR' in r and r.get('SMoSR').id == 'SMoSR' and resselt_amd.get('SMoSR') is r.tail['SMoSR']
    meta, _ = load_golden('registry_claims')
    assert 'SMoSR' in meta['order']


def test_the_tail_tier_is_general():
    """Any number of entries, in insertion order, behind everything else; re-registering replaces in place; an id another tier already
    holds stays where it is; registering without ``tail`` moves it into the walk."""
    from resselt_amd.factory import Architecture, KeyCondition
    from resselt_amd.registry import Registry

    class Stub(Architecture):
        def load(self, state_dict):
            raise AssertionError('never built')

    mk = lambda uid: Stub(uid=uid, detect=KeyCondition.has_all(uid))  # noqa: E731
    r = Registry()
    r.add(mk('S'))
    r.add(mk('T1'), tail=True)
    r.add(mk('A'), after=True)
    r.add(mk('T2'), tail=True)
    assert list(r.tail) == ['T1', 'T2'] and [x.id for x in r.every()] == ['S', 'A', 'T1', 'T2'] and [x.id for x in r.consulted()] == ['S', 'A']
    assert len(r) == 1 and 'T2' in r and r.get('T2').id == 'T2'
    t1 = mk('T1')
    r.add(t1, tail=True)
    assert list(r.tail) == ['T1', 'T2'] and r.get('T1') is t1
    r.add(mk('A'), tail=True)  # already in ``after``: replaced there
    assert 'A' not in r.tail and list(r.after) == ['A']
    r.add(mk('T2'))  # moved into the walk on request
    assert list(r.tail) == ['T1'] and list(r.store) == ['S', 'T2']
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        r.load_from_state_dict({'nothing': torch.zeros(1)})


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
    ('FlexNet', lambda: synth.flexnet_state_dict(dim=16, num_blocks=(1,))), ('MoESR', lambda: synth.moesr_state_dict(dim=16, n_blocks=1, n_block=1, scale=2)),
]  # fmt: skip


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('SMoSR').detect(sd)
    claims = [a.id for a in internal_registry.every() if a.detect(sd)]
    assert claims and claims[0] == uid and 'SMoSR' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'SMoSR'


def test_every_other_registered_architecture_has_a_checkpoint_above():
    assert {a.id for a in internal_registry.every()} - {'SMoSR'} == {u for u, _ in OTHERS}


def test_the_refusals():
    load = lambda **kw: resselt_amd.load_from_state_dict(dict(synth.smosr_state_dict(**dict(SMALL, **kw))))  # noqa: E731
    # what the reference itself cannot run (checked on it): the module is built from hyper-parameters alone, as its loader would
    with pytest.raises(NotImplementedError, match='rep = 1 with the dysample head'):
        SMoSR(**SMALL, rep=True, upsampler='dysample')
    with pytest.raises(NotImplementedError, match='mid_dim == dim \\+ in_ch \\* scale\\^2'):
        SMoSR(**SMALL, upsampler='dysample', upsampler_mid_dim=16 + 3 * 4)
    meta = torch.tensor([254, 4, 2, 28, 3, 28, 4, 0], dtype=torch.uint8)  # such a checkpoint has its DySample at upsampler.0
    sd = {k: v for k, v in synth.smosr_state_dict(**SMALL).items() if not k.startswith('upsampler.')} | {'upsampler.MetaUpsample': meta}
    with pytest.raises(NotImplementedError, match='KeyError on upsampler.2.end_conv.weight'):
        resselt_amd.load_from_state_dict(sd)
    with pytest.raises(NotImplementedError, match='conv head with scale 2'):
        SMoSR(**SMALL, upsampler='conv', scale=2)
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        load(dim=20)
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8 up to 128'):
        load(dim=136)
    with pytest.raises(NotImplementedError, match='pa_up needs mid_dim a multiple of 8'):
        load(upsampler='pa_up', upsampler_mid_dim=20)
    with pytest.raises(NotImplementedError, match='pa_up needs mid_dim a multiple of 8 up to 128'):
        load(upsampler='pa_up', upsampler_mid_dim=136)
    assert isinstance(load(upsampler='pa_up', upsampler_mid_dim=24, scale=3), SMoSR)
    with pytest.raises(ValueError, match='invalid Upsample'):
        SMoSR(upsampler='bicubic')


@pytest.mark.parametrize('shape', [(1, 3, 2, 9), (1, 3, 9, 2), (1, 3, 1, 1)])
def test_inputs_under_three_pixels_raise(shape):
    """The plan builder refuses before anything is allocated or launched (F.pad(..., 'reflect') of 2 needs 3 pixels)."""
    m = resselt_amd.load_from_state_dict(dict(synth.smosr_state_dict(**SMALL)))
    with pytest.raises(RuntimeError, match='too small for the reflect padding'):
        m._build_plan(Plan('cpu'), {}, shape, torch.float32, m.products)
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m._build_plan(Plan('cpu'), {}, (1, 1, 9, 9), torch.float32, m.products)


def test_plan_output_crop_origin():
    """``Plan.output(crop_origin=...)``: the window ``take_output`` keeps starts there; without it, at the map's origin as before."""
    p = Plan('cpu')
    y = p.output((1, 2, 8, 10), torch.float32, crop=(4, 6), crop_origin=(2, 3))
    y.copy_(torch.arange(160.0).reshape(1, 2, 8, 10))
    want = y[:, :, 2:6, 3:9].clone()
    assert torch.equal(p.take_output(), want)
    p = Plan('cpu')
    y = p.output((1, 2, 8, 10), torch.float32, crop=(4, 6))
    y.zero_()
    assert p.take_output().shape == (1, 2, 4, 6) and p._crop_origin is None


def test_file_round_trips(tmp_path):
    from safetensors.torch import save_file

    sd = synth.smosr_state_dict(**SMALL, rep=True, upsampler='pa_up', upsampler_mid_dim=8, seed=9)
    torch.save(dict(sd), tmp_path / 'm.pth')
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'm.safetensors'))
    for name in ('m.pth', 'm.safetensors'):
        m = resselt_amd.load_from_file(str(tmp_path / name))
        assert isinstance(m, SMoSR) and m.parameters_info.name == 'SMoSR'
        got = m.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], v) and got[k].dtype == v.dtype for k, v in sd.items())
