"""MoSR / MoSRv2 without a GPU: the CPU oracle against the reference's vectors, detection and inferred metadata, the registry order, the
claimants of the other synthetic state dicts, and the exactness of the pack-time folds (channel re-layout of the gated block, GPS mean)."""

import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mosr_oracle as O
import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.archs.mosr.arch import fold_gps, gate_layout, pad_dw, relayout_gate
from resselt_amd.utils import synth

NAMES = golden_names('mosr_') + golden_names('mosrv2_')


def _sd(meta):
    fn = synth.mosr_state_dict if meta['arch'] == 'mosr' else synth.mosrv2_state_dict
    return fn(seed=meta['seed'], **meta['synth'])


def test_fixtures_exist():
    assert len(golden_names('mosr_')) >= 7 and len(golden_names('mosrv2_')) >= 11


@pytest.mark.parametrize('name', NAMES)
def test_oracle_matches_reference_vectors(name):
    meta, arr = load_golden(name)
    sd = _sd(meta)
    with torch.no_grad():
        if meta['arch'] == 'mosr':
            y = O.mosr_forward(sd, arr['x'], meta['synth'].get('upsampler', 'ps'), meta['metadata']['upscale'])
        else:
            y = O.mosrv2_forward(sd, arr['x'], meta['synth'].get('upsampler', 'pixelshuffledirect'), meta['metadata']['upscale'])
    assert y.shape == arr['y'].shape
    assert (y - arr['y']).abs().max().item() <= 1e-5 * arr['y'].abs().max().item()


@pytest.mark.parametrize('name', NAMES)
def test_claimed_with_reference_metadata(name):
    meta, _ = load_golden(name)
    sd = _sd(meta)
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert meta['claimed_by'] == {'mosr': 'MoSR', 'mosrv2': 'MoSRv2'}[meta['arch']]
    assert type(m).__name__ == meta['metadata']['cls']
    assert vars(m.parameters_info) == {k: meta['metadata'][k] for k in ('in_channels', 'out_channels', 'upscale', 'name')}
    m.load_state_dict(sd, strict=True)
    assert set(m.state_dict()) == set(sd)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert m.resolved_precision() == 'bf16x3' and not m.supports_u8 and not m.global_statistics


def test_mosrv2_unshuffle_x1_loads_as_x1():
    sd = synth.mosrv2_state_dict(scale=1, n_block=1, dim=32, unshuffle_mod=True, seed=5)
    assert sd['gblocks.1.weight'].shape[1] == 48
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert type(m).__name__ == 'MoSRv2' and m.parameters_info.upscale == 1 and m.unshuffle == 4 and m.s_int == 4
    y = O.mosrv2_forward(sd, synth.synth_input((1, 3, 9, 10), 5), 'pixelshuffledirect', 1)
    assert y.shape == (1, 3, 9, 10)


def test_registry_order_follows_reference():
    from resselt_amd.archs import internal_registry

    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'registry_claims.npz'))
    ref = json.loads(str(z['meta']))['order']
    order = list(internal_registry.store.keys())
    assert [u for u in ref if u in order] == order
    assert order.index('Compact') < order.index('MoSR') < order.index('CuGAN')
    assert order.index('PLKSR') < order.index('MoSRv2') < order.index('RTMoSR')


@pytest.mark.parametrize('make, uid', [
    (lambda: synth.rrdbnet_state_dict(nb=1), 'ESRGAN'),
    (lambda: synth.compact_state_dict(num_conv=2), 'Compact'),
    (lambda: synth.rtmosr_state_dict(), 'RTMoSR'),
    (lambda: synth.plksr_state_dict(n_blocks=1, dim=32), 'PLKSR'),
    (lambda: synth.realplksr_state_dict(n_blocks=1, dim=32), 'PLKSR'),
    (lambda: synth.cugan_state_dict(), 'CuGAN'),
    (lambda: synth.span_state_dict(), 'SPAN'),
    (lambda: synth.spanplus_state_dict(), 'spanplus'),
    (lambda: synth.spanpp_state_dict(), 'SpanPP'),
])  # fmt: skip
def test_other_state_dicts_keep_their_claimant(make, uid):
    from resselt_amd.archs import internal_registry

    sd = make()
    got = next(a.id for a in internal_registry.store.values() if a.detect(sd))
    assert got == uid


def _gate_cpu(x, w1, b1, w2, groups_fn):
    """fc1 -> mish(g) * groups_fn(rest) -> fc2 (f64)."""
    f = F.conv2d(x, w1, b1, padding=1)
    h = f.shape[1] // 2
    return F.conv2d(F.mish(f[:, :h]) * groups_fn(f[:, h:]), w2, None, padding=1)


@pytest.mark.parametrize('dim, hidden, groups', [
    (40, 60, [(20, (1, 1)), (40, (7, 7))]),                                               # MoSR dim 40: i = 20, c = 40
    (48, 72, [(48, (1, 1)), (24, (5, 5))]),                                               # MoSR conv_ratio 0.5
    (40, 60, [(20, (1, 1)), (25, (1, 1)), (5, (3, 3)), (5, (1, 11)), (5, (11, 1))]),      # MoSRv2 dim 40: gc = 5
    (48, 72, [(24, (1, 1)), (30, (1, 1)), (6, (3, 3)), (6, (1, 11)), (6, (11, 1))]),      # MoSRv2 dim 48: gc = 6
])  # fmt: skip
def test_gate_relayout_is_exact(dim, hidden, groups):
    g = torch.Generator().manual_seed(dim + hidden)
    d = torch.float64
    w1, b1 = torch.randn(2 * hidden, dim, 3, 3, generator=g, dtype=d), torch.randn(2 * hidden, generator=g, dtype=d)
    w2 = torch.randn(dim, hidden, 3, 3, generator=g, dtype=d)
    dws = [(torch.randn(c, 1, *k, generator=g, dtype=d), torch.randn(c, generator=g, dtype=d)) if k != (1, 1) else None for c, k in groups]
    x = torch.randn(2, dim, 13, 17, generator=g, dtype=d)

    def ref_groups(r):
        out, c0 = [], 0
        for (c, k), dw in zip(groups, dws):
            out.append(r[:, c0 : c0 + c] if dw is None else F.conv2d(r[:, c0 : c0 + c], dw[0], dw[1], padding=(k[0] // 2, k[1] // 2), groups=c))
            c0 += c
        return torch.cat(out, 1)

    perm, i_planes, segs, planes = gate_layout(groups)
    assert sorted(set(perm)) == perm and len(perm) == hidden
    assert all(p % 8 == 0 for p in [8 * i_planes] + [perm[s[3]] for s in segs])  # every group starts on a plane boundary
    pw1, pb1, pw2 = relayout_gate(w1, b1, w2, perm, planes)
    assert pw1.shape[0] == 16 * planes and pw2.shape[1] == 8 * planes
    conv_dws = [dw for dw in dws if dw is not None]

    def padded_groups(r):  # what rsa_gated_dwconv computes on the padded planes
        out = [r[:, : 8 * i_planes]]
        c0 = 8 * i_planes
        for (pl, kh, kw, _, _), (w, b) in zip(segs, conv_dws):
            wt, bt = pad_dw(w, b, pl)
            out.append(F.conv2d(r[:, c0 : c0 + 8 * pl], wt.to(d).reshape(8 * pl, 1, kh, kw), bt.to(d), padding=(kh // 2, kw // 2), groups=8 * pl))
            c0 += 8 * pl
        return torch.cat(out, 1)

    for w, b in conv_dws:  # (pad_dw keeps f32 weights: compare against the f32-rounded unpadded form)
        w.copy_(w.float().double())
        b.copy_(b.float().double())
    ref = _gate_cpu(x, w1, b1, w2, ref_groups)
    got = _gate_cpu(x, pw1, pb1, pw2, padded_groups)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_gps_fold_is_exact():
    g = torch.Generator().manual_seed(9)
    d = torch.float64
    s, out_ch, dim = 3, 3, 16
    w, b = torch.randn(s * s * out_ch * 8, dim, 3, 3, generator=g, dtype=d), torch.randn(s * s * out_ch * 8, generator=g, dtype=d)
    x = torch.randn(2, dim, 11, 9, generator=g, dtype=d)
    y = F.conv2d(x, w, b, padding=1)
    ref = F.pixel_shuffle(y.reshape(2, 8, -1, 11, 9).mean(1), s)
    wf, bf = fold_gps(w, b)
    got = F.pixel_shuffle(F.conv2d(x, wf, bf, padding=1), s)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


@pytest.mark.parametrize('make, what', [
    (lambda: synth.mosr_state_dict(n_block=1, dim=36), 'multiple of 8'),
    (lambda: synth.mosr_state_dict(n_block=1, dim=32, kernel_size=13), 'not compiled'),
    (lambda: synth.mosrv2_state_dict(n_block=1, dim=36), 'multiple of 8'),
])  # fmt: skip
def test_unsupported_shapes_raise(make, what):
    with pytest.raises(NotImplementedError, match=what):
        resselt_amd.load_from_state_dict(dict(make()))
