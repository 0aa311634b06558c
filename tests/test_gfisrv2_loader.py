"""CPU checks of the GFISRv2 loader: detection (each of the reference's 22 keys is needed), its place in the registry (membership and
relative order only: the tier it sits in is open-ended), the inferred hyper-parameters and metadata against what the reference's loader
inferred, the parameter tree against the reference module's state_dict (names with the rotating attribute names, order, shapes, dtypes),
that no other architecture's checkpoint changes owner, the refusals, the tiny-input probe and the file round trips.  On the commit before
GFISRv2 every load here raises ``ArchitectureNotFound``."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.gfisrv2 import DETECTION_KEYS
from resselt_amd.archs.gfisrv2.arch import GFISRV2, branch_order, gfisr_gate_layout
from resselt_amd.engine.base import Plan
from resselt_amd.utils import synth

NAMES = [n for n in golden_names('gfisrv2_') if n != 'gfisrv2_tiny_probe']
SMALL = dict(dim=16, n_blocks=1, scale=2)


def _sd(meta):
    return synth.gfisrv2_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures_cover_what_the_issue_lists():
    metas = [load_golden(n)[0] for n in NAMES]
    hy = [m['hyper'] for m in metas]
    assert len(NAMES) == 9
    assert {h['dim'] for h in hy} >= {16, 24, 48, 64} and {h['scale'] for h in hy} == {1, 2, 3, 4}
    assert {h['upsampler'] for h in hy} == {'conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample'}
    assert any(h['n_blocks'] >= 5 for h in hy) and any((h['dim'], h['n_blocks']) == (48, 24) for h in hy)
    assert any(h['in_nc'] == 1 and h['out_nc'] == 1 for h in hy)
    shapes = [tuple(load_golden(n)[1]['x'].shape) for n in NAMES]
    assert any(s[0] == 2 for s in shapes)
    parity = {(s[2] % 2, s[3] % 2) for s in shapes}
    assert {(1, 1), (0, 0), (1, 0)} <= parity


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert meta['claims'] == ['GFISRV2']  # what the whole reference registry said
    claims = [a.id for a in internal_registry.order() if a.detect(sd)]
    assert claims == ['GFISRV2']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, GFISRV2)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'GFISRV2'
    hy = meta['hyper']
    assert (m.in_ch, m.out_ch, m.dim, m.scale, m.n_block, m.head, m.mid_dim) == (
        hy['in_nc'], hy['out_nc'], hy['dim'], hy['scale'], hy['n_blocks'], hy['upsampler'], hy['mid_dim'])  # fmt: skip
    assert hy['pixel_unshuffle'] is False and m.hidden == int(hy['expansion_ratio'] * hy['dim']) == sd['gfisr_body.0.fc1.weight'].shape[0] // 2
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
    assert {k: str(v.dtype) for k, v in got.items() if v.dtype != torch.float32} == meta['dtypes'] == {'upscale.MetaUpsample': 'torch.uint8'}
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    hy = meta['hyper']
    index = ('conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up').index(hy['upsampler'])
    assert [int(v) for v in got['upscale.MetaUpsample']] == [3, index, hy['scale'], hy['dim'], hy['out_nc'], hy['mid_dim'], 4]
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'gfisr_body.0.conv.pconv.rn.scale'})


def test_the_attribute_names_rotate_with_the_block_index():
    sd = synth.gfisrv2_state_dict(dim=16, n_blocks=5, scale=2)
    for i, slot in enumerate(('pconv', 'dwconv_h', 'dwconv_w', 'dwconv_hw', 'pconv')):  # block 4 wraps
        assert f'gfisr_body.{i}.conv.{slot}.fdc.weight' in sd and sd[f'gfisr_body.{i}.conv.{slot}.fdc.weight'].shape == (20, 20, 1, 1)
        assert [name for name, kind in branch_order(i) if kind is None] == [slot]
        assert sum(f'gfisr_body.{i}.conv.' in k and k.endswith('fdc.weight') for k in sd) == 1
    assert [k for _, k in branch_order(1)] == [(3, 3), (1, 11), (11, 1), None]
    assert sd['gfisr_body.1.conv.pconv.weight'].shape == (2, 1, 3, 3) and sd['gfisr_body.1.conv.dwconv_w.weight'].shape == (2, 1, 11, 1)


@pytest.mark.parametrize('dim,hidden', [(16, 42), (24, 64), (48, 128), (48, 72), (64, 170), (16, 16)])
@pytest.mark.parametrize('shift', [0, 1, 2, 3, 4])
def test_gate_layout(dim, hidden, shift):
    """Every branch starts on a plane boundary, the FourierUnit right behind ``i``, the depthwise segments in channel order behind it; the
    permutation is injective and keeps every reference channel."""
    perm, i_pl, f_pl, segs, planes, f_src = gfisr_gate_layout(hidden, dim, shift)
    gc, cf, i_ch = dim // 8, dim - 3 * (dim // 8), hidden - dim
    assert len(perm) == hidden == len(set(perm)) and max(perm) < 8 * planes
    assert perm[:i_ch] == list(range(i_ch)) and i_pl == (i_ch + 7) // 8 and f_pl == (cf + 7) // 8
    assert planes == i_pl + f_pl + 3 * ((gc + 7) // 8)
    order = branch_order(shift)
    src, pos, seen = i_ch, 8 * (i_pl + f_pl), []
    for name, kind in order:
        width = cf if kind is None else gc
        if kind is None:
            assert perm[src : src + width] == list(range(8 * i_pl, 8 * i_pl + cf)) and f_src == src - i_ch
        else:
            assert perm[src : src + width] == list(range(pos, pos + gc))
            seen.append((kind[0], kind[1], name))
            pos += 8 * ((gc + 7) // 8)
        src += width
    assert [(kh, kw, name) for _, kh, kw, name in segs] == seen


def test_each_detection_key_is_needed():
    arch = internal_registry.get('GFISRV2')
    sd = synth.gfisrv2_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 22 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        less = {k: v for k, v in sd.items() if k != drop}
        assert not arch.detect(less), drop
        with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
            resselt_amd.load_from_state_dict(less)
    assert arch.detect({k: v for k, v in sd.items() if k != 'in_to_dim.weight'})  # not a detection key


def test_registry_position():
    """GFISRV2 is consulted after everything ``every()`` yields, and none of the older tiers and iterators knows it.  Membership and relative
    order only: the tier is open-ended, and the next architecture goes into it too."""
    r = internal_registry
    assert all('GFISRV2' not in t for t in (r.store, r.late, r.last, r.after, r.tail)) and 'GFISRV2' in r.rest
    every = [a.id for a in r.every()]
    order = [a.id for a in r.order()]
    assert 'GFISRV2' not in every and 'GFISRV2' not in [a.id for a in r] and 'GFISRV2' not in [a.id for a in r.walk()]
    assert 'GFISRV2' not in [a.id for a in r.consulted()] and len(r) == len(r.store) + len(r.late)
    assert order[: len(every)] == every and order[len(every) :] == list(r.rest) and order.index('GFISRV2') >= len(every)
    assert 'GFISRV2' in r and r.get('GFISRV2').id == 'GFISRV2' and resselt_amd.get('GFISRV2') is r.rest['GFISRV2']
    meta, _ = load_golden('registry_claims')
    assert 'GFISRV2' in meta['order']


def test_the_rest_tier_is_general():
    """Any number of entries, in insertion order, behind everything else; re-registering replaces in place; an id another tier already
    holds stays where it is; registering without ``rest`` moves it into the walk."""
    from resselt_amd.factory import Architecture, KeyCondition
    from resselt_amd.registry import Registry

    class Stub(Architecture):
        def load(self, state_dict):
            raise AssertionError('never built')

    mk = lambda uid: Stub(uid=uid, detect=KeyCondition.has_all(uid))  # noqa: E731
    r = Registry()
    r.add(mk('S'))
    r.add(mk('R1'), rest=True)
    r.add(mk('T'), tail=True)
    r.add(mk('R2'), rest=True)
    assert list(r.rest) == ['R1', 'R2'] and [x.id for x in r.order()] == ['S', 'T', 'R1', 'R2'] and [x.id for x in r.every()] == ['S', 'T']
    assert len(r) == 1 and 'R2' in r and r.get('R2').id == 'R2'
    r1 = mk('R1')
    r.add(r1, rest=True)
    assert list(r.rest) == ['R1', 'R2'] and r.get('R1') is r1
    r.add(mk('T'), rest=True)  # already in ``tail``: replaced there
    assert 'T' not in r.rest and list(r.tail) == ['T']
    r.add(mk('R2'))  # moved into the walk on request
    assert list(r.rest) == ['R1'] and list(r.store) == ['S', 'R2']
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        r.load_from_state_dict({'nothing': torch.zeros(1)})


OTHERS = [
    ('eimn', lambda: synth.eimn_state_dict(num_stages=1)), ('ESRGAN', lambda: synth.rrdbnet_state_dict(nb=1)), ('spanplus', lambda: synth.spanplus_state_dict(blocks=(1,))),
    ('SPAN', lambda: synth.span_state_dict()), ('SwinIR', lambda: synth.swinir_state_dict()), ('Compact', lambda: synth.compact_state_dict(num_conv=2)),
    ('dat', lambda: synth.dat_state_dict()), ('SpanPP', lambda: synth.spanpp_state_dict()), ('HAT', lambda: synth.hat_state_dict()),
    ('RTMoSR', lambda: synth.rtmosr_state_dict()), ('DRCT', lambda: synth.drct_state_dict()), ('PLKSR', lambda: synth.plksr_state_dict()),
    ('PLKSR', lambda: synth.realplksr_state_dict()), ('CuGAN', lambda: synth.cugan_state_dict()), ('MoSR', lambda: synth.mosr_state_dict(n_block=1)),
    ('MoSRv2', lambda: synth.mosrv2_state_dict(n_block=1)), ('MoSRv2', lambda: synth.mosrv2_state_dict(n_block=1, rms_norm=True)),
    ('RGT', lambda: synth.rgt_state_dict()), ('FDAT', lambda: synth.fdat_state_dict()),
    ('OmniSR', lambda: synth.omnisr_state_dict()), ('ATD', lambda: synth.atd_state_dict()), ('RCAN', lambda: synth.rcan_state_dict(n_resgroups=1, n_resblocks=1)),
    ('GateR', lambda: synth.gater_state_dict(dim=24, num_blocks=(1,) * 7)), ('RHA', lambda: synth.rha_state_dict(dim=16, group_blocks=1, res_blocks=1)),
    ('FlexNet', lambda: synth.flexnet_state_dict(dim=16, num_blocks=(1,))), ('MoESR', lambda: synth.moesr_state_dict(dim=16, n_blocks=1, n_block=1, scale=2)),
    ('SMoSR', lambda: synth.smosr_state_dict(dim=16, n_mb=1)),
]  # fmt: skip


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('GFISRV2').detect(sd)
    claims = [a.id for a in internal_registry.order() if a.detect(sd)]
    assert claims and claims[0] == uid and 'GFISRV2' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'GFISRV2'


def test_every_architecture_consulted_before_it_has_a_checkpoint_above():
    order = [a.id for a in internal_registry.order()]
    assert set(order[: order.index('GFISRV2')]) <= {u for u, _ in OTHERS}


def test_the_refusals():
    load = lambda **kw: resselt_amd.load_from_state_dict(dict(synth.gfisrv2_state_dict(**dict(SMALL, **kw))))  # noqa: E731
    # a pixel_unshuffle checkpoint, as the reference would write one (in_to_dim.1 over 4 * 4 * in_nc channels, MetaUpsample scale 4)
    sd = synth.gfisrv2_state_dict(**dict(SMALL, scale=4))
    w, b = sd.pop('in_to_dim.weight'), sd.pop('in_to_dim.bias')
    sd['in_to_dim.1.weight'], sd['in_to_dim.1.bias'] = w.repeat(1, 4, 1, 1), b
    assert internal_registry.get('GFISRV2').detect(sd)
    with pytest.raises(NotImplementedError, match='pixel_unshuffle checkpoints are not built'):
        resselt_amd.load_from_state_dict(sd)
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        load(dim=20)
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8 up to 128'):
        load(dim=136)
    with pytest.raises(NotImplementedError, match='hidden = int\\(expansion_ratio \\* dim\\) must be at least dim'):
        load(expansion_ratio=0.75)
    for head in ('transpose+conv', 'lda', 'pa_up'):
        with pytest.raises(NotImplementedError, match='head is not built'):
            GFISRV2(**SMALL, upsampler=head)
        assert isinstance(GFISRV2(dim=16, n_blocks=1, scale=1, upsampler=head), GFISRV2)  # at scale 1 every mode is the one convolution
    with pytest.raises(NotImplementedError, match='hidden widths must be multiples of 8'):
        load(upsampler='pixelshuffle', mid_dim=20)
    with pytest.raises(ValueError, match='invalid Upsample'):
        GFISRV2(upsampler='bicubic')
    assert isinstance(load(dim=128, expansion_ratio=1.0), GFISRV2)


def test_tiny_inputs_raise_where_the_reference_does():
    meta, _ = load_golden('gfisrv2_tiny_probe')
    probe = {tuple(p['size']): p['raises'] for p in meta['probe']}
    assert set(probe) == {(1, 1), (1, 2), (2, 1), (1, 3), (3, 1)} and probe[(1, 1)] == 'RuntimeError' and probe[(2, 1)] is None
    m = resselt_amd.load_from_state_dict(dict(synth.gfisrv2_state_dict(seed=meta['seed'], **meta['synth'])))
    for (h, w), raises in probe.items():
        if raises is None:
            continue  # (these sizes run on the GPU: tests/test_gfisrv2_gpu.py)
        assert raises == 'RuntimeError'
        with pytest.raises(RuntimeError, match='view_as_complex'):  # before anything is allocated or launched
            m._build_plan(Plan('cpu'), {}, (1, 3, h, w), torch.float32, m.products)
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m._build_plan(Plan('cpu'), {}, (1, 1, 9, 9), torch.float32, m.products)


def test_file_round_trips(tmp_path):
    from safetensors.torch import save_file

    sd = synth.gfisrv2_state_dict(**SMALL, upsampler='dysample', mid_dim=24, seed=9)
    torch.save(dict(sd), tmp_path / 'm.pth')
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'm.safetensors'))
    for name in ('m.pth', 'm.safetensors'):
        m = resselt_amd.load_from_file(str(tmp_path / name))
        assert isinstance(m, GFISRV2) and m.parameters_info.name == 'GFISRV2'
        got = m.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], v) and got[k].dtype == v.dtype for k, v in sd.items())
