"""CPU checks of the GFISR (v1) loader: detection (each of the reference's 16 keys is needed), its place in the registry (behind LAWFFT, every
older tier and iterator unchanged), the inferred hyper-parameters and metadata against what the reference's loader inferred, the parameter
tree against the reference module's state_dict (names with the rotating attribute names, order, shapes, dtypes; the dead ``weight.0``
tensors of the FourierUnit included), that no other architecture's checkpoint changes owner, the two loader quirks against the probe, the
five-way gate layout, the refusals and the too-small grids.  On the commit before GFISR every load here raises ``ArchitectureNotFound``."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.gfisr import DETECTION_KEYS
from resselt_amd.archs.gfisr.arch import GFISR, branch_order, gfisr1_gate_layout, padded_size
from resselt_amd.engine.base import Plan
from resselt_amd.utils import synth
from test_gfisrv2_loader import OTHERS as OLDER

NAMES = [n for n in golden_names('gfisr_') if n != 'gfisr_probe']
LOADED = [n for n in NAMES if not load_golden(n)[0]['direct']]
DIRECT = [n for n in NAMES if load_golden(n)[0]['direct']]
SMALL = dict(dim=16, n_blocks=1, scale=2)


def _sd(meta):
    return synth.gfisr_state_dict(seed=meta['seed'], **meta['synth'])


def test_fixtures_cover_what_the_issue_lists():
    hy = [load_golden(n)[0]['hyper'] for n in LOADED]
    assert len(LOADED) == 10 and len(DIRECT) == 2
    assert {h['dim'] for h in hy} >= {8, 16, 24, 32, 48, 64} and {h['scale'] for h in hy} == {1, 2, 3, 4}
    assert {h['upsampler'] for h in hy} == {'conv', 'pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample'}
    assert any((h['dim'], h['n_blocks']) == (48, 24) for h in hy) and any(h['n_blocks'] == 6 for h in hy)  # the default; five rotations and a wrap
    assert any(h['in_nc'] == 1 and h['out_nc'] == 1 for h in hy) and any(h['fft_mode'] is False for h in hy) and any(h['expansion_ratio'] == 1.5 for h in hy)
    assert all(h['upsample_dim'] == 32 and 'mid_dim' not in h for h in hy)  # the quirk: the loader never hands ``mid_dim`` over
    shapes = [tuple(load_golden(n)[1]['x'].shape) for n in LOADED]
    assert any(s[0] == 2 for s in shapes) and {(s[2] % 2, s[3] % 2) for s in shapes} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for n in DIRECT:
        meta, arr = load_golden(n)
        assert meta['claims'] == [] and meta['synth']['pixel_unshuffle'] is True
        u = 4 // meta['synth']['scale']
        assert tuple(-(-s // u) for s in arr['x'].shape[2:]) == (4, 5)  # the feature grid


@pytest.mark.parametrize('name', LOADED)
def test_detection_and_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert meta['claims'] == ['GFISR']  # what the whole reference registry said
    assert [a.id for a in internal_registry.full() if a.detect(sd)] == ['GFISR']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, GFISR)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    assert pi.name == 'GFISR'
    hy = meta['hyper']
    assert (m.in_ch, m.out_ch, m.dim, m.scale, m.out_scale, m.n_block, m.head, m.fft_mode, m.unshuffle) == (
        hy['in_nc'], hy['out_nc'], hy['dim'], hy['scale'], hy['scale'], hy['n_blocks'], hy['upsampler'], hy['fft_mode'], 1)  # fmt: skip
    assert hy['pixel_unshuffle'] is False and m.mid_dim == 32
    assert m.hidden == int(hy['expansion_ratio'] * hy['dim']) == sd['net.0.fc1.weight'].shape[0] // 2
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'fp16') and m.global_statistics is True
    assert m.macs_per_input_pixel() > 0


@pytest.mark.parametrize('name', NAMES)
def test_parameter_tree_equals_the_reference_modules(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    assert list(sd) == list(meta['state_dict']) and {k: list(v.shape) for k, v in sd.items()} == meta['state_dict']
    if meta['direct']:
        m = GFISR(**meta['synth'])
        m.load_state_dict(dict(sd))
        assert m.unshuffle == 4 // meta['synth']['scale'] and (m.out_scale, m.scale) == (meta['synth']['scale'], 4)
    else:
        m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert list(got) == list(meta['state_dict'])  # names and registration order of the reference module
    assert all(list(got[k].shape) == v for k, v in meta['state_dict'].items())
    assert {k: str(v.dtype) for k, v in got.items() if v.dtype != torch.float32} == meta['dtypes'] == {'dim_to_out.MetaUpsample': 'torch.uint8'}
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    dead = [k for k in got if '.weight.0.' in k]
    assert len(dead) == (2 * m.n_block if m.fft_mode else 0)  # the one-channel softmax branch: checkpoint keys that round-trip
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'net.0.fc2.bias'})
    if dead:
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if k != dead[0]})


def test_the_dead_branch_takes_no_part_in_the_arithmetic():
    """A softmax over ONE channel is 1.0 whatever the convolution in front of it gives: the oracle, which evaluates the branch, returns the
    same bits for other ``weight.0`` tensors, and the engine never reads them."""
    import gfisr_oracle as O

    sd = synth.gfisr_state_dict(**SMALL, seed=3)
    x = synth.synth_input((1, 3, 5, 6), 3).double()
    other = {k: (v * -7.0 + 2.0 if '.weight.0.' in k else v) for k, v in sd.items()}
    with torch.no_grad():
        assert torch.equal(O.gfisr_forward(sd, x), O.gfisr_forward(other, x))


def test_the_attribute_names_rotate_with_the_block_index():
    sd = synth.gfisr_state_dict(dim=16, n_blocks=6, scale=2)
    for i, slot in enumerate(('fsas', 'dwconv_h', 'dwconv_w', 'dwconv_hw', 'pconv', 'fsas')):  # block 5 wraps
        assert sd[f'net.{i}.conv.{slot}.fdc.weight'].shape == (4, 4, 1, 1) and sd[f'net.{i}.conv.{slot}.weight.0.weight'].shape == (1, 4, 1, 1)
        assert [name for name, kind in branch_order(i) if kind == 'fourier'] == [slot]
        assert sum(f'net.{i}.conv.' in k and k.endswith('fdc.weight') for k in sd) == 1
        identity = next(name for name, kind in branch_order(i) if kind == 'identity')
        assert not any(k.startswith(f'net.{i}.conv.{identity}.') for k in sd)  # the identity registers nothing
    assert [k for _, k in branch_order(1)] == [(3, 3), (1, 11), (11, 1), 'fourier', 'identity']
    assert sd['net.1.conv.pconv.weight'].shape == (2, 1, 3, 3) and sd['net.1.conv.dwconv_w.weight'].shape == (2, 1, 11, 1)
    off = synth.gfisr_state_dict(dim=16, n_blocks=6, scale=2, fft_mode=False)
    assert not any('.fdc.' in k or '.ln.' in k for k in off) and len(off) == len(sd) - 8 * 6


@pytest.mark.parametrize('dim,hidden', [(8, 21), (16, 42), (24, 64), (48, 128), (48, 72), (64, 170), (128, 341), (16, 16)])
@pytest.mark.parametrize('shift', [0, 1, 2, 3, 4, 5])
def test_gate_layout(dim, hidden, shift):
    """Every branch starts on a plane boundary whatever its rotated position -- ``i``, the identity, the FourierUnit, then the depthwise
    segments in channel order -- and the permutation is injective and keeps every reference channel."""
    perm, i_pl, d_pl, f_pl, segs, planes = gfisr1_gate_layout(hidden, dim, shift)
    gc, i_ch = dim // 8, hidden - dim
    idc, g_pl = dim - 4 * gc, (gc + 7) // 8
    assert len(perm) == hidden == len(set(perm)) and max(perm) < 8 * planes
    assert perm[:i_ch] == list(range(i_ch)) and i_pl == (i_ch + 7) // 8 and d_pl == (idc + 7) // 8 and f_pl == g_pl
    assert planes == i_pl + d_pl + 4 * g_pl
    src, pos, seen = i_ch, 8 * (i_pl + d_pl + f_pl), []
    for name, kind in branch_order(shift):
        width = idc if kind == 'identity' else gc
        got = perm[src : src + width]
        assert got[0] % 8 == 0 and got == list(range(got[0], got[0] + width))  # plane-aligned and contiguous
        if kind == 'identity':
            assert got[0] == 8 * i_pl
        elif kind == 'fourier':
            assert got[0] == 8 * (i_pl + d_pl)
        else:
            assert got[0] == pos
            seen.append((g_pl, kind[0], kind[1], name))
            pos += 8 * g_pl
        src += width
    assert src == hidden and segs == seen and sorted((kh, kw) for _, kh, kw, _ in segs) == [(1, 11), (3, 3), (11, 1)]
    assert gfisr1_gate_layout(hidden, dim, shift + 5) == (perm, i_pl, d_pl, f_pl, [(p, kh, kw, n) for p, kh, kw, n in segs], planes)


def test_each_detection_key_is_needed():
    arch = internal_registry.get('GFISR')
    sd = synth.gfisr_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 16 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        less = {k: v for k, v in sd.items() if k != drop}
        assert not arch.detect(less), drop
        with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
            resselt_amd.load_from_state_dict(less)
    assert arch.detect({k: v for k, v in sd.items() if k != 'net.0.conv.fsas.ln.weight'})  # not a detection key


def test_registry_position():
    """GFISR is consulted behind LAWFFT, after everything ``order()`` yields, and none of the older tiers and iterators knows it."""
    r = internal_registry
    assert all('GFISR' not in t for t in (r.store, r.late, r.last, r.after, r.tail, r.rest)) and list(r.more) == ['GFISR']
    assert list(r.rest) == ['GFISRV2', 'FIGSR', 'LAWFFT']
    order, full = [a.id for a in r.order()], [a.id for a in r.full()]
    assert 'GFISR' not in order and full == order + ['GFISR'] and full.index('GFISR') == full.index('LAWFFT') + 1
    for it in (r, r.walk(), r.consulted(), r.every()):
        assert 'GFISR' not in [a.id for a in it]
    assert len(r) == len(r.store) + len(r.late)
    assert 'GFISR' in r and r.get('GFISR').id == 'GFISR' and resselt_amd.get('GFISR') is r.more['GFISR']


def test_the_more_tier_is_general():
    from resselt_amd.factory import Architecture, KeyCondition
    from resselt_amd.registry import Registry

    class Stub(Architecture):
        def load(self, state_dict):
            raise AssertionError('never built')

    mk = lambda uid: Stub(uid=uid, detect=KeyCondition.has_all(uid))  # noqa: E731
    r = Registry()
    r.add(mk('S'))
    r.add(mk('M1'), more=True)
    r.add(mk('R'), rest=True)
    r.add(mk('M2'), more=True)
    assert list(r.more) == ['M1', 'M2'] and [x.id for x in r.full()] == ['S', 'R', 'M1', 'M2'] and [x.id for x in r.order()] == ['S', 'R']
    m1 = mk('M1')
    r.add(m1, more=True)
    assert list(r.more) == ['M1', 'M2'] and r.get('M1') is m1
    r.add(mk('R'), more=True)  # already in ``rest``: replaced there
    assert 'R' not in r.more and list(r.rest) == ['R']
    r.add(mk('M2'))  # moved into the walk on request
    assert list(r.more) == ['M1'] and list(r.store) == ['S', 'M2']
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        r.load_from_state_dict({'nothing': torch.zeros(1)})


OTHERS = OLDER + [
    ('GFISRV2', lambda: synth.gfisrv2_state_dict(dim=16, n_blocks=1, scale=2)), ('FIGSR', lambda: synth.figsr_state_dict(dim=32, n_blocks=2, scale=2)),
    ('LAWFFT', lambda: synth.lawfft_state_dict(n_rblock=1, n_mblock=2)),
]  # fmt: skip


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('GFISR').detect(sd)
    claims = [a.id for a in internal_registry.full() if a.detect(sd)]
    assert claims and claims[0] == uid and 'GFISR' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'GFISR'


def test_every_architecture_consulted_before_it_has_a_checkpoint_above():
    full = [a.id for a in internal_registry.full()]
    assert set(full[: full.index('GFISR')]) <= {u for u, _ in OTHERS}


def test_the_loader_quirks_match_the_probe():
    meta, _ = load_golden('gfisr_probe')
    # 1. ``upsample_dim=`` lands in **kwargs: mid_dim is always 32, and a head of another mid_dim fails in the strict load_state_dict
    q = meta['mid_dim']
    assert q['raises'] == 'RuntimeError' and 'loading state_dict' in q['message'] and q['synth']['mid_dim'] != 32
    with pytest.raises(RuntimeError, match='size mismatch'):
        resselt_amd.load_from_state_dict(dict(synth.gfisr_state_dict(seed=meta['seed'], **q['synth'])))
    # 2. detection needs in_to_dim.weight: a pixel_unshuffle checkpoint is never detected, although load() has a branch for it
    q = meta['pixel_unshuffle']
    assert q['raises'] == 'ArchitectureNotFound' and q['claims'] == []
    sd = synth.gfisr_state_dict(seed=meta['seed'], **q['synth'])
    assert 'in_to_dim.1.weight' in sd and not internal_registry.get('GFISR').detect(sd)
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        resselt_amd.load_from_state_dict(dict(sd))
    # the branch itself infers what the reference's infers: scale 4 from the MetaUpsample buffer, so no unshuffle stage, and the strict load fails
    with pytest.raises(RuntimeError):
        m = internal_registry.get('GFISR').load(sd)
        assert m.unshuffle == 1 and m.in_ch == 3
        m.load_state_dict(dict(sd))


def test_the_refusals():
    load = lambda **kw: resselt_amd.load_from_state_dict(dict(synth.gfisr_state_dict(**dict(SMALL, **kw))))  # noqa: E731
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        load(dim=20)
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8 up to 128'):
        load(dim=136)
    with pytest.raises(NotImplementedError, match='hidden = int\\(expansion_ratio \\* dim\\) must be at least dim'):
        load(expansion_ratio=0.75)
    for kw in (dict(in_nc=9), dict(in_nc=0)):
        with pytest.raises(NotImplementedError, match='1 to 8 input channels'):
            GFISR(**SMALL, **kw)
    for kw in (dict(out_nc=9), dict(out_nc=0)):
        with pytest.raises(NotImplementedError, match='1 to 8 output channels'):
            GFISR(**SMALL, **kw)
    for head in ('transpose+conv', 'lda', 'pa_up'):
        with pytest.raises(NotImplementedError, match='head is not built'):
            GFISR(**SMALL, upsampler=head, pixel_unshuffle=False)
        with pytest.raises(NotImplementedError, match='head is not built'):
            GFISR(dim=16, n_blocks=1, scale=1, upsampler=head)  # pixel_unshuffle (the default): the head runs at x4
        assert isinstance(GFISR(dim=16, n_blocks=1, scale=1, upsampler=head, pixel_unshuffle=False), GFISR)  # at scale 1 every mode is the one convolution
    with pytest.raises(ValueError, match='invalid Upsample'):
        GFISR(upsampler='bicubic')
    assert isinstance(load(dim=128, expansion_ratio=1.0), GFISR)
    m = GFISR()  # the module's defaults: pixel_unshuffle=True does nothing at x4
    assert (m.dim, m.n_block, m.scale, m.unshuffle, m.hidden, m.gc) == (48, 24, 4, 1, 128, 6)


def test_too_small_grids_raise_where_the_reference_does():
    meta, _ = load_golden('gfisr_probe')
    probe = {tuple(p['size']): p['raises'] for p in meta['probe']}
    assert probe == {(3, 3): 'RuntimeError', (3, 4): 'RuntimeError', (4, 3): 'RuntimeError', (4, 4): None, (4, 5): None, (5, 5): None}
    assert all('Padding size should be less than' in p['message'] for p in meta['probe'] if p['raises'])
    m = resselt_amd.load_from_state_dict(dict(_sd(meta)))
    for (h, w), raises in list(probe.items()) + [((2, 5), 'RuntimeError'), ((5, 2), 'RuntimeError'), ((1, 8), 'RuntimeError')]:
        if raises is None:
            continue  # (these sizes run on the GPU: tests/test_gfisr_gpu.py)
        with pytest.raises(RuntimeError, match='Padding size should be less than'):  # before anything is allocated or launched
            m._build_plan(Plan('cpu'), {}, (1, 3, h, w), torch.float32, m.products)
    with pytest.raises(RuntimeError, match='expects 3 input channels'):
        m._build_plan(Plan('cpu'), {}, (1, 1, 9, 9), torch.float32, m.products)
    assert padded_size(4, 5) == (8, 10) and padded_size(5, 7) == (10, 12) and padded_size(33, 70) == (38, 74)
    # a pixel_unshuffle model counts its FEATURE grid: 7 x 9 at x2 is 4 x 5 and runs, 5 x 9 is 3 x 5 and raises
    pu = GFISR(dim=16, n_blocks=1, scale=2, pixel_unshuffle=True)
    with pytest.raises(RuntimeError, match='a 3x5 feature grid'):
        pu._build_plan(Plan('cpu'), {}, (1, 3, 5, 9), torch.float32, pu.products)


def test_file_round_trips(tmp_path):
    from safetensors.torch import save_file

    sd = synth.gfisr_state_dict(**SMALL, upsampler='dysample', seed=9)
    torch.save(dict(sd), tmp_path / 'm.pth')
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'm.safetensors'))
    for name in ('m.pth', 'm.safetensors'):
        m = resselt_amd.load_from_file(str(tmp_path / name))
        assert isinstance(m, GFISR) and m.parameters_info.name == 'GFISR'
        got = m.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], v) and got[k].dtype == v.dtype for k, v in sd.items())
