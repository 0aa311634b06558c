"""CPU checks of the GateRv2 loader: detection (each of the reference's keys is needed; a one-level checkpoint is not detected), its place in
the registry (behind GateRV3, in ``Registry.beyond``; every older tier and iterator unchanged), the inferred hyper-parameters and metadata
against what the reference's loader inferred (above x1, where the reference's loader raises ``KeyError``: against the generator's
arguments), the parameter tree against the reference module's state_dict (names, order, shapes, dtypes), that no other architecture's
checkpoint or fixture changes owner, the refusals with their messages, the probe findings one by one and the sizes that raise.  On the
commit before GateRv2 every load here raises ``ArchitectureNotFound``."""

import pytest
import torch

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs import internal_registry
from resselt_amd.archs.gaterv2 import DETECTION_KEYS, GateRV2Arch
from resselt_amd.archs.gaterv2.arch import GateRV2
from resselt_amd.engine.base import Plan
from resselt_amd.utils import synth
from test_gaterv3_loader import OTHERS as OLDER

NAMES = [n for n in golden_names('gaterv2_') if n != 'gaterv2_probe']
SMALL = dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1)
OTHERS = OLDER + [('GateRV3', lambda: synth.gaterv3_state_dict(dim=8, enc_blocks=(1, 1), dec_blocks=(1, 1), num_latent=1, span_blocks=1))]


def _sd(meta):
    return synth.gaterv2_state_dict(seed=meta['seed'], **meta['synth'])


def test_loading_a_synthetic_checkpoint():
    m = resselt_amd.load_from_state_dict(dict(synth.gaterv2_state_dict()))
    assert isinstance(m, GateRV2) and m.parameters_info.name == 'GateRv2'
    assert (m.dim, m.enc_blocks, m.dec_blocks, m.num_latent, m.scale, m.pad, m.latent_width, m.qk) == (48, (2, 2, 4, 6), (2, 2, 2, 2), 10, 1, 16, 768, 48)
    assert m.meta_gated_count() == 22 and m.expected_launches() == 1 + 220 + 8 + 80 + 12 + 1


def test_fixtures_cover_what_the_issue_lists():
    metas = [load_golden(n)[0] for n in NAMES]
    hy = [m['hyper'] for m in metas]
    shapes = [tuple(load_golden(n)[1]['x'].shape) for n in NAMES]
    assert any((h['dim'], h['enc_blocks'], h['dec_blocks'], h['num_latent'], h['scale']) == (48, [2, 2, 4, 6], [2, 2, 2, 2], 10, 1) and s[2:] == (17, 35)
               for h, s in zip(hy, shapes))  # fmt: skip
    assert {(h['dim'] << len(h['enc_blocks'])) // 16 for h in hy} >= {2, 6, 16, 48}  # m: not a multiple of 8, and whole planes
    tokens = [(-(-s[2] // (1 << len(h['enc_blocks'])))) * (-(-s[3] // (1 << len(h['enc_blocks'])))) for h, s in zip(hy, shapes)]
    assert any(128 < t and t % 128 for t in tokens)  # two chunks, the last one ragged
    assert {(h['upsample'], h['scale']) for h in hy if h['scale'] != 1} == {('pixelshuffledirect', 2), ('pixelshuffledirect', 3), ('pixelshuffle', 4), ('pixelshuffle', 3),
                                                                            ('nearest+conv', 4), ('nearest+conv', 3), ('dysample', 2), ('dysample', 3), ('conv', 2)}  # fmt: skip
    assert any(h['in_ch'] == 1 for h in hy) and any(s[0] == 2 for s in shapes)
    assert any(len(set(h['enc_blocks'])) > 1 and h['enc_blocks'] != h['dec_blocks'] and len(h['enc_blocks']) == 3 for h in hy)
    pads = [((1 << len(h['enc_blocks'])), s[2:]) for h, s in zip(hy, shapes)]
    assert any(P in s for P, s in pads) and any(P + 1 in s for P, s in pads)  # a side that is exactly P; side P + 1: a pad of P - 1, the largest there is
    assert all(m['scale_attribute_set'] == (m['hyper']['scale'] != 1) and ('KeyError' in m['via']) == (m['hyper']['scale'] != 1) for m in metas)


@pytest.mark.parametrize('name', NAMES)
def test_detection_and_metadata(name):
    meta, arr = load_golden(name)
    sd = _sd(meta)
    assert meta['claims'] == ['GateRv2']  # what the whole reference registry said
    assert [a.id for a in internal_registry.consultation() if a.detect(sd)] == ['GateRv2']  # no other registered architecture claims it
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, GateRV2)
    pi, md = m.parameters_info, meta['metadata']
    assert (pi.in_channels, pi.out_channels, pi.upscale, pi.name) == (md['in_channels'], md['out_channels'], md['upscale'], md['name'])
    hy = meta['hyper']  # x1: every argument the reference's loader handed over; above: the generator's arguments
    got = GateRV2Arch.hyperparameters(sd)
    assert {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in got.items()} == hy
    assert (m.in_ch, m.dim, list(m.enc_blocks), list(m.dec_blocks), m.num_latent, m.scale) == (hy['in_ch'], hy['dim'], hy['enc_blocks'], hy['dec_blocks'], hy['num_latent'], hy['scale'])
    if m.scale != 1:
        assert (m.upsampler, m.mid_dim, pi.upscale) == (hy['upsample'], hy['upsample_mid_dim'], hy['scale'])
        h, w = arr['x'].shape[-2:]
        full = (h * m.scale, w * m.scale) if m.upsampler != 'conv' else (min(h * m.scale, -(-h // m.pad) * m.pad), min(w * m.scale, -(-w // m.pad) * m.pad))
        assert tuple(arr['y'].shape[-2:]) == full  # the FULL image, not the reference module's H x W corner
    assert m.resolved_precision() == 'bf16x3' and m.precisions == ('bf16x3', 'bf16', 'fp16') and m.global_statistics is True
    assert m.macs_per_input_pixel() > 0 and m.pad == 1 << len(hy['enc_blocks'])


@pytest.mark.parametrize('name', NAMES)
def test_parameter_tree_equals_the_reference_modules(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    want = meta['state_dict']
    assert list(sd) == list(want) and all(list(v.shape) == want[k] for k, v in sd.items())
    m = resselt_amd.load_from_state_dict(dict(sd))
    got = m.state_dict()
    assert list(got) == list(want)  # names and registration order of the reference module
    assert all(list(got[k].shape) == v for k, v in want.items())
    assert {k: str(v.dtype) for k, v in got.items() if v.dtype != torch.float32} == meta['dtypes']
    for k, v in sd.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'decode.0.shor.bias'})


def test_each_detection_key_is_needed():
    meta, _ = load_golden('gaterv2_probe')
    assert meta['detection_keys'] == meta['detection_keys_needed'] == 110  # the reference's detector needs each of these keys, and there are 110
    arch = internal_registry.get('GateRv2')
    sd = synth.gaterv2_state_dict(**SMALL)
    assert len(DETECTION_KEYS) == len(set(DETECTION_KEYS)) == 110 and arch.detect(sd)
    for drop in DETECTION_KEYS:
        assert not arch.detect({k: v for k, v in sd.items() if k != drop}), drop
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        resselt_amd.load_from_state_dict({k: v for k, v in sd.items() if k != DETECTION_KEYS[0]})


def test_registry_position():
    """GateRv2 is consulted behind GateRV3, after everything ``full()`` yields, and none of the older tiers and iterators knows it."""
    r = internal_registry
    assert all('GateRv2' not in t for t in (r.store, r.late, r.last, r.after, r.tail, r.rest, r.more)) and 'GateRv2' in r.beyond
    full, walk = [a.id for a in r.full()], [a.id for a in r.consultation()]
    assert 'GateRv2' not in full and walk[: len(full)] == full and walk.index('GateRv2') > walk.index('GateRV3')
    for it in (r, r.walk(), r.consulted(), r.every(), r.order(), r.full()):
        assert 'GateRv2' not in [a.id for a in it]
    assert 'GateRv2' in r and r.get('GateRv2').id == 'GateRv2' and resselt_amd.get('GateRv2') is r.beyond['GateRv2']
    assert set(walk[: walk.index('GateRv2')]) <= {u for u, _ in OTHERS}  # every architecture consulted before it has a checkpoint below


@pytest.mark.parametrize('uid,make', OTHERS, ids=[f'{u}-{i}' for i, (u, _) in enumerate(OTHERS)])
def test_other_checkpoints_keep_their_owner(uid, make):
    sd = make()
    assert not internal_registry.get('GateRv2').detect(sd)
    claims = [a.id for a in internal_registry.consultation() if a.detect(sd)]
    assert claims and claims[0] == uid and 'GateRv2' not in claims
    assert type(resselt_amd.load_from_state_dict(dict(sd))).__name__ != 'GateRV2'


def test_no_fixture_of_another_family_is_claimed():
    """Every golden fixture that records the keys of its state dict: none but GateRv2's own satisfies the detector."""
    arch = internal_registry.get('GateRv2')
    seen = 0
    for name in golden_names(''):
        meta, _ = load_golden(name)
        if not isinstance(meta, dict) or not isinstance(meta.get('state_dict'), dict):
            continue
        seen += 1
        assert arch.detect({k: None for k in meta['state_dict']}) == name.startswith('gaterv2_'), name
    assert seen > len(NAMES)


def test_the_probe_findings():
    meta, arr = load_golden('gaterv2_probe')
    # 1. the reference's loader reads the wrong key above x1; this one loads the checkpoint
    q = meta['loader_above_x1']
    assert q['raises'] == 'KeyError' and 'to_img.MetaUpsample' in q['message'] and q['claims'] == ['GateRv2']
    case, _ = load_golden(q['case'])
    sd = _sd(case)
    assert 'upsample.MetaUpsample' in sd and 'to_img.MetaUpsample' not in sd
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert isinstance(m, GateRV2) and m.parameters_info.upscale == m.scale == 2
    # 2. the reference module keeps scale = 1: its output is the H x W corner
    q = meta['scale_crop']
    assert (q['scale_attribute'], q['scale_argument']) == (1, 2) and q['y_unmodified'] == q['x'] and tuple(arr['y_crop_unmodified'].shape) == tuple(arr['x_crop'].shape)
    # 3. more encoder than decoder levels: the reference loads it and raises in forward
    q = meta['dec_ne_enc']
    assert q['load']['raises'] is None and q['forward']['raises'] == 'RuntimeError'
    # 4. one level is not detected (the detector asks for encode.1 and decode.1)
    q = meta['one_level']
    assert q['raises'] == 'ArchitectureNotFound' and q['claims'] == []
    with pytest.raises(resselt_amd.registry.ArchitectureNotFound):
        resselt_amd.load_from_state_dict(dict(synth.gaterv2_state_dict(seed=meta['seed'], **q['synth'])))
    # 5. a 'conv' head above x1 does not upsample: the padded map, cropped to at most H scale x W scale
    q = meta['conv_above_x1']
    assert q['y_unmodified'] == q['x'] and q['y_scale_set'][-2:] == [8, 8] and q['corner_equal'] is True
    assert tuple(load_golden(q['case'])[1]['y'].shape) == tuple(q['y_scale_set'])
    # 6. nothing else in the reference's registry claims a GateRv2 state dict
    assert meta['x1_claims'] == ['GateRv2']


def test_the_refusals():
    load = lambda **kw: resselt_amd.load_from_state_dict(dict(synth.gaterv2_state_dict(**dict(SMALL, **kw))))  # noqa: E731
    meta, _ = load_golden('gaterv2_probe')
    with pytest.raises(NotImplementedError, match='2 decoder levels for 3 encoder levels'):
        resselt_amd.load_from_state_dict(dict(synth.gaterv2_state_dict(seed=meta['seed'], **meta['dec_ne_enc']['synth'])))
    with pytest.raises(NotImplementedError, match='dim must be a multiple of 8'):
        load(dim=12)
    # a latent stage above 1024 channels and a MetaGated above 512 are the same models (the latent stage is twice as wide): one message
    with pytest.raises(NotImplementedError, match='widest MetaGated.* = 1024, exceeds 512'):
        GateRV2(dim=64, enc_blocks=(1,) * 5, dec_blocks=(1,) * 5)
    with pytest.raises(NotImplementedError, match='widest MetaGated.* = 520, exceeds 512'):
        GateRV2(dim=520, enc_blocks=(1,), dec_blocks=(1,))
    with pytest.raises(NotImplementedError, match='widest MetaGated.* = 528, exceeds 512'):
        GateRV2(dim=264, enc_blocks=(1, 1), dec_blocks=(1, 1))
    wide = GateRV2(dim=512, enc_blocks=(1,), dec_blocks=(1,), num_latent=1)  # the limits themselves: a 512-wide MetaGated, a 1024-wide latent stage
    assert (wide.latent_width, wide.qk) == (1024, 64)
    assert isinstance(GateRV2(), GateRV2) and GateRV2().latent_width == 768  # the default model
    with pytest.raises(NotImplementedError, match="head's hidden widths must be multiples of 8"):
        load(scale=2, upsample='pixelshuffle', upsample_mid_dim=12)
    assert isinstance(load(scale=2, upsample='dysample', upsample_mid_dim=12), GateRV2)  # UniUpsample v1's DySample does not use mid_dim
    with pytest.raises(ValueError, match='invalid Upsample'):
        GateRV2(**SMALL, scale=2, upsample='bicubic')
    for up in ('pixelshuffle', 'nearest+conv'):
        with pytest.raises(ValueError, match='scale 5 is not supported'):
            GateRV2(**SMALL, scale=5, upsample=up)
    assert isinstance(GateRV2(**SMALL, scale=1, upsample='bicubic'), GateRV2)  # at scale 1 the head is never built, as in the reference
    for kw in (dict(in_ch=9), dict(in_ch=0)):
        with pytest.raises(NotImplementedError, match='1 to 8 input channels'):
            GateRV2(**SMALL, **kw)
    with pytest.raises(NotImplementedError, match='at least one block'):
        GateRV2(dim=8, enc_blocks=(1, 0), dec_blocks=(1, 1), num_latent=1)


def test_sizes_raise_where_the_reference_does():
    meta, _ = load_golden('gaterv2_probe')
    probe = {(p['model'], tuple(p['size'])): p['raises'] for p in meta['probe']}
    assert {k: v for k, v in probe.items() if k[0] == 'p4' and k[1][0] <= 3} == {('p4', (1, 5)): 'RuntimeError', ('p4', (2, 7)): 'RuntimeError', ('p4', (3, 9)): None}
    assert probe[('p16', (8, 19))] == probe[('p16', (19, 8))] == 'RuntimeError' and probe[('p16', (9, 21))] is None and probe[('p16', (21, 9))] is None
    assert all('Padding size should be less than' in p['message'] for p in meta['probe'] if p['raises'])
    for tag, kw in meta['synth'].items():
        m = resselt_amd.load_from_state_dict(dict(synth.gaterv2_state_dict(seed=meta['seed'], **kw)))
        for (model, (h, w)), raises in probe.items():
            if model != tag:
                continue
            if raises is None:  # the rule accepts it (these sizes run on the GPU: tests/test_gaterv2_gpu.py)
                assert all((m.pad - s % m.pad) % m.pad < s for s in (h, w))
                continue
            with pytest.raises(RuntimeError, match='Padding size should be less than'):  # before anything is allocated or launched
                m._build_plan(Plan('cpu'), {}, (1, 3, h, w), torch.float32, m.products)
        with pytest.raises(RuntimeError, match='expects 3 input channels'):
            m._build_plan(Plan('cpu'), {}, (1, 1, 32, 32), torch.float32, m.products)


def test_file_round_trips(tmp_path):
    from safetensors.torch import save_file

    sd = synth.gaterv2_state_dict(**SMALL, scale=2, upsample='dysample', upsample_mid_dim=16, seed=9)
    torch.save(dict(sd), tmp_path / 'm.pth')
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'm.safetensors'))
    for name in ('m.pth', 'm.safetensors'):
        m = resselt_amd.load_from_file(str(tmp_path / name))
        assert isinstance(m, GateRV2) and m.parameters_info.name == 'GateRv2' and m.parameters_info.upscale == 2
        got = m.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], v) and got[k].dtype == v.dtype for k, v in sd.items())
