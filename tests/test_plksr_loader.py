"""PLKSR / RealPLKSR loading without a GPU: detection, inferred metadata, strict state dicts, the pack-time folds of the sparse
large-kernel variants, the shapes the engine refuses, and the tiling warning of whole-image statistics."""

import warnings

import pytest
import torch
import torch.nn.functional as F

import resselt_amd
from helpers import golden_names, load_golden
from resselt_amd.engine import plk
from resselt_amd.utils import synth

NAMES = golden_names('plksr_') + golden_names('realplksr_')


def _state_dict(meta):
    fn = synth.plksr_state_dict if meta['arch'] == 'plksr' else synth.realplksr_state_dict
    return fn(seed=meta['seed'], **meta['synth'])


def test_fixtures_exist():
    assert len(golden_names('plksr_')) >= 6 and len(golden_names('realplksr_')) >= 8


@pytest.mark.parametrize('name', NAMES)
def test_claimed_with_reference_metadata(name):
    meta, _ = load_golden(name)
    sd = _state_dict(meta)
    m = resselt_amd.load_from_state_dict(dict(sd))
    assert meta['claimed_by'] == 'PLKSR'
    assert type(m).__name__ == meta['metadata']['cls']
    assert vars(m.parameters_info) == {k: meta['metadata'][k] for k in ('in_channels', 'out_channels', 'upscale', 'name')}
    m.load_state_dict(sd, strict=True)
    assert set(m.state_dict()) == set(sd)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k


def test_registry_order_follows_reference():
    from resselt_amd.archs import internal_registry

    order = list(internal_registry.store.keys())
    assert order.index('Compact') < order.index('PLKSR') < order.index('RTMoSR') < order.index('spanplus')


def test_rect_sparse_fold_is_exact():
    g = torch.Generator().manual_seed(0)
    pdim, k = 8, 17
    n = k // 3
    ws = [torch.randn(pdim, pdim, *s, generator=g, dtype=torch.float64) for s in ((k, n), (n, k), (n, n))]
    bs = [torch.randn(pdim, generator=g, dtype=torch.float64) for _ in range(3)]
    x = torch.randn(1, pdim, 23, 29, generator=g, dtype=torch.float64)
    ref = sum(F.conv2d(x, w, b, padding=(w.shape[2] // 2, w.shape[3] // 2)) for w, b in zip(ws, bs))
    wf, bf = plk.fold_rect_sparse(ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], k)
    assert wf.shape == (pdim, pdim, k, k)
    got = F.conv2d(x, wf, bf, padding=k // 2)
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


def test_sparse_fold_is_exact():
    g = torch.Generator().manual_seed(1)
    pdim, k = 8, 17
    convs = [(torch.randn(pdim, pdim, 5, 5, generator=g, dtype=torch.float64), torch.randn(pdim, generator=g, dtype=torch.float64), d) for d in (1, 2, 3, 4)]
    x = torch.randn(2, pdim, 31, 26, generator=g, dtype=torch.float64)
    ref = sum(F.conv2d(x, w, b, padding=2 * d, dilation=d) for w, b, d in convs)
    wf, bf = plk.fold_sparse(convs, k)
    got = F.conv2d(x, wf, bf, padding=k // 2)
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize('kw, what', [
    (dict(dim=36), 'dim must be a multiple of 8'),
    (dict(dim=40, split_ratio=0.25), 'pdim'),
    (dict(kernel_size=16), 'kernel_size'),
    (dict(kernel_size=33), 'kernel_size'),
])  # fmt: skip
def test_unsupported_shapes_raise(kw, what):
    with pytest.raises(NotImplementedError, match=what):
        resselt_amd.load_from_state_dict(synth.realplksr_state_dict(n_blocks=1, **kw))


def test_unsupported_input_channels_raise():
    sd = synth.realplksr_state_dict(dim=32, n_blocks=1)
    sd['feats.0.weight'] = torch.zeros(32, 1, 3, 3)
    sd['feats.3.weight'], sd['feats.3.bias'] = torch.zeros(16, 32, 3, 3), torch.zeros(16)
    with pytest.raises(NotImplementedError, match='input channels'):
        resselt_amd.load_from_state_dict(sd)


def _fake_forward(scale):
    return lambda x: F.interpolate(x, scale_factor=scale, mode='nearest')


def test_tiling_warns_for_whole_image_statistics():
    from resselt_amd.tiling import upscale_tiled

    m = resselt_amd.load_from_state_dict(synth.realplksr_state_dict(dim=32, n_blocks=1, upscale=2))
    assert m.global_statistics
    m.forward = _fake_forward(2)  # the tiler's logic only: no GPU here
    x = torch.rand(1, 3, 40, 40)
    with pytest.warns(RuntimeWarning, match='whole image'):
        upscale_tiled(m, x, 2, (16, 16), halo=4, check=False)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        upscale_tiled(m, x, 2, (64, 64), halo=4, check=False)  # one tile: no warning


def test_tiling_does_not_warn_for_compact():
    from resselt_amd.tiling import upscale_tiled

    m = resselt_amd.load_from_state_dict(synth.compact_state_dict(num_feat=16, num_conv=1, upscale=2))
    assert not getattr(m, 'global_statistics', False)
    m.forward = _fake_forward(2)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        upscale_tiled(m, torch.rand(1, 3, 40, 40), 2, (16, 16), halo=4, check=False)


@pytest.mark.parametrize('lk_type, k', [('PLK', 9), ('PLK', 31), ('SparsePLK', 17), ('RectSparsePLK', 9), ('RectSparsePLK', 17), ('RectSparsePLK', 27)])
def test_model_fold_matches_unfolded_oracle(lk_type, k):
    """The dense kernel the model packs (its own fold of the checkpoint's branches) against the oracle's UNFOLDED large-kernel layer --
    every dilated / rectangular branch run as its own convolution -- on images larger and smaller than the kernel."""
    from oracle.plksr import large_kernel

    sd = synth.plksr_state_dict(dim=32, n_blocks=1, upscale=2, kernel_size=k, lk_type=lk_type, seed=5)
    m = resselt_amd.load_from_state_dict(dict(sd))
    sd64 = {key: v.to(torch.float64) for key, v in sd.items()}
    w, b = m._lk_weights(sd64, 1)
    kk = m.kernel_size
    assert w.shape == (8, 8, kk, kk)
    g = torch.Generator().manual_seed(k)
    for hw in ((23, 29), (5, 7), (1, 12)):
        x = torch.randn(1, 32, *hw, generator=g, dtype=torch.float64)
        ref = large_kernel(sd64, 'feats.1.lk', x)
        got = F.conv2d(x[:, :8], w, b, padding=kk // 2)
        assert torch.equal(ref[:, 8:], x[:, 8:])
        assert (got - ref[:, :8]).abs().max() <= 1e-12 * ref.abs().max(), (lk_type, k, hw)
