"""MoSR, MoSRv2, RGT, FDAT, OmniSR, ATD, RCAN, GateR, EIMN, RHA, FlexNet, MoESR, SMoSR and GFISRv2 (fourteen families) on the GPU against their float64 CPU oracles
(tests/<arch>_oracle.py through helpers.oracle_forward) at the shapes their fixtures do not reach:

1. consecutive sizes: every side the oracle accepts from 1 up to ``top`` (2 P + 1 for a pad multiple P, 9 without padding, further where
   the smallest legal side lies above that) on either axis, the other side fixed at another residue -- every pad from none to the largest
   legal one, one window, two windows plus a row;
2. acceptance: over the same range the engine raises exactly where the oracle (whose behaviour is the reference's) raises, before any launch;
   the configurations the README lists as not built (SMoSR's conv head above x1 and rep = 1 with dysample, GFISRv2's transpose+conv, lda and
   pa_up heads above x1) and GFISRv2's 1 x 1 input (refused by the reference, not by the oracle's dense DFT) raise before any launch too;
3. batch isolation: three images of clearly different statistics at a size odd in both axes, the error reported per image;
4. every head of the multi-head families at the largest legal pad in H and a pad of 1 in W, and transposed;
5. plan cache (A, B, A again) and precision switch (a one-product mode and back): bit-equal;
6. one multi-tile frame of 70 x 150 per family;
7. fp16 / bf16 tensors in and out, non-contiguous and channels_last inputs (the same bits as the contiguous copy, the input untouched).

Every case calls the model twice: the first output is compared with the oracle on the same values, the second must be bit-equal (the cached
plan).  ATD goes through atd_trajectory.run_on_engine_trajectory (the oracle forced along the engine's recorded permutations), on inputs
whose float64 oracle decisions all have a top-two margin of at least 5 TAU (``guarded_input``), so that no decision may differ; the 70 x 150
frame has too many decisions for that and keeps the 0.2 % cap of test_atd_gpu.py.

Tolerance (asserted): that of tests/fuzz_parity.py, max-abs <= 3e-4 / 2e-3 / 1.2e-2 * max(1, |ref|max) for fp32 / fp16 / bf16 tensors, in
'auto' and 'bf16x3' (three products).  Each case also prints ``err / family bar`` on a MEASURE line, the family bar being the constant of
the family's own test_<arch>_gpu.py (imported, set there at about twice the error of its fixtures); it is not asserted.  On a failure the
place of the largest error is printed: image, channel, row, column, and whether it lies in the last pad multiple of rows or columns.

Worst err / family bar per family, measured on an MI355X (profiles/newer_archs_sweep_measure.txt has every MEASURE line): MoSR 0.04,
MoSRv2 0.005, RGT 0.013, FDAT 0.03, OmniSR 0.024, ATD 0.037 (those six bars are relative, 2e-4 or 3e-4 of max(1, |y|max)); RCAN 0.46,
GateR 0.54, EIMN 0.40, RHA 0.71, FlexNet 0.57 (absolute bars at about twice a fixture's error); MoESR 0.05, SMoSR 0.39, GFISRv2 0.03 (relative,
2e-4).  No case exceeds its family bar.

``Case``, ``_check`` and the bodies of the acceptance, batch and layout tests live in tests/sweep_common.py, which
test_original_archs_sweep_gpu.py uses for the ten original families as well.
"""

import pytest
import torch

import resselt_amd
from helpers import load_golden
from resselt_amd.archs.gfisrv2.arch import SAMPLE_MODS3
from resselt_amd.archs.smosr.arch import SAMPLE_MODS as SMOSR_MODS
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth
from sweep_common import Case as CommonCase
from sweep_common import _check, _input, _largest_pad_and_pad_one, _status_ok, acceptance, batch_of_three, dtypes_and_layouts  # noqa: F401  (_status_ok: autouse)
from test_atd_gpu import _tol as atd_bar
from test_eimn_gpu import TOL_BF16X3 as EIMN_BAR
from test_fdat_gpu import _tol as fdat_bar
from test_flexnet_gpu import TOL_BF16X3 as FLEXNET_BAR
from test_gater_gpu import TOL_BF16X3 as GATER_BAR
from test_gfisrv2_gpu import MODEL_REL as GFISRV2_REL
from test_moesr_gpu import MODEL_REL as MOESR_REL
from test_mosr_gpu import _tol as mosr_bar
from test_omnisr_gpu import _tol as omnisr_bar
from test_rcan_gpu import TOL_BF16X3 as RCAN_BAR
from test_rgt_gpu import _tol as rgt_bar
from test_rha_gpu import TOL_BF16X3 as RHA_BAR
from test_smosr_gpu import MODEL_REL as SMOSR_REL

pytestmark = pytest.mark.gpu

FAMILY_BAR = {'mosr': mosr_bar, 'mosrv2': mosr_bar, 'rgt': rgt_bar, 'fdat': fdat_bar, 'omnisr': omnisr_bar, 'atd': atd_bar,
              'rcan': lambda ref: RCAN_BAR, 'gater': lambda ref: GATER_BAR, 'eimn': lambda ref: EIMN_BAR, 'rha': lambda ref: RHA_BAR,
              'flexnet': lambda ref: FLEXNET_BAR, 'moesr': lambda ref: MOESR_REL * max(1.0, ref.abs().max().item()),
              'smosr': lambda ref: SMOSR_REL * max(1.0, ref.abs().max().item()), 'gfisrv2': lambda ref: GFISRV2_REL * max(1.0, ref.abs().max().item())}  # fmt: skip


# --------------------------------------------------------------------------------------------------------------------- configurations
# name -> (family, synth keywords, pad multiple P in input pixels, top of the swept range, the other side: legal, of another residue)
#   * no padding (MoSR, EIMN, RCAN without unshuffle_mod): sides 1..9 -- the single pixel and sides below the largest depthwise kernel;
#   * RGT pads its windows to max(split_size) = 4 but RG-SA needs 16 rows and columns: 16..25; OmniSR's ESA needs a padded side of 16,
#     with window 4 that is 13..22.
CONFIGS = {
    'mosr': ('mosr', dict(upscale=2, n_block=2, dim=32, upsampler='ps', kernel_size=7), 0, 9, 6),
    'mosrv2_u2': ('mosrv2', dict(scale=2, n_block=2, dim=32, upsampler='pixelshuffledirect', unshuffle_mod=True), 2, 5, 7),
    'mosrv2_u4': ('mosrv2', dict(scale=1, n_block=2, dim=32, upsampler='pixelshuffledirect', unshuffle_mod=True), 4, 9, 7),
    'rgt': ('rgt', dict(embed_dim=32, depth=(2,), num_heads=(2,), split_size=(2, 4), upscale=2), 4, 25, 19),
    'fdat': ('fdat', dict(scale=2, embed_dim=32, num_groups=1, depth_per_group=2, num_heads=4, window_size=4, upsampler_type='pixelshuffledirect'), 4, 9, 7),
    'fdat_unshuffle': ('fdat', dict(scale=2, embed_dim=32, num_groups=1, depth_per_group=2, num_heads=4, window_size=4, upsampler_type='pixelshuffledirect',
                                    unshuffle_mod=True), 8, 17, 11),
    'omnisr_w4': ('omnisr', dict(num_feat=32, window_size=4, up_scale=2), 4, 22, 15),
    'omnisr_w8': ('omnisr', dict(num_feat=32, window_size=8, up_scale=2), 8, 17, 13),
    'atd': ('atd', dict(embed_dim=48, depths=(2,), num_heads=(4,), window_size=8, num_tokens=64, reducted_dim=8, upscale=2,
                        upsampler='pixelshuffledirect'), 8, 17, 11),
    'rcan48': ('rcan', dict(scale=2, n_resgroups=1, n_resblocks=2, n_feats=48), 0, 9, 6),
    'rcan64_unshuffle': ('rcan', dict(scale=2, n_resgroups=1, n_resblocks=2, n_feats=64, unshuffle_mod=True), 2, 9, 7),
    'gater': ('gater', dict(dim=24, num_blocks=(1,) * 7, latent_att=True), 8, 17, 13),
    'eimn': ('eimn', dict(embed_dims=32, scale=2, num_stages=2), 0, 9, 6),
    'rha': ('rha', dict(dim=32, scale=2, down_list=(2, 1), window_size=4, group_blocks=1, res_blocks=2), 8, 17, 11),
    'rha_p16': ('rha', dict(dim=32, scale=2, down_list=(4, 2), window_size=4, group_blocks=1, res_blocks=2), 16, 33, 21),
    'flexnet': ('flexnet', dict(dim=32, num_blocks=(1, 1), scale=2), 8, 17, 13),
    'moesr': ('moesr', dict(scale=2, dim=32, n_blocks=1, n_block=1), 2, 9, 7),  # (the MSG stage runs at half resolution: reflect pad to 2)
    'smosr': ('smosr', dict(scale=2, dim=32, n_mb=1), 0, 9, 6),  # (reflect pad of 2 all round: sides from 3)
    'gfisrv2': ('gfisrv2', dict(scale=2, dim=16, n_blocks=2), 0, 9, 6),  # (every size but 1 x 1; the dense DFT has a table per side)
}  # fmt: skip
ALL = list(CONFIGS)
ONE_PER_FAMILY = ['mosr', 'mosrv2_u4', 'rgt', 'fdat_unshuffle', 'omnisr_w8', 'atd', 'rcan64_unshuffle', 'gater', 'eimn', 'rha', 'flexnet',
                  'moesr', 'smosr', 'gfisrv2']  # fmt: skip


def _meta(family, kw):
    """What helpers.oracle_forward needs besides the state dict."""
    meta = dict(arch=family)
    if family == 'mosr':
        meta.update(upsampler=kw['upsampler'], upscale=kw['upscale'])
    elif family == 'mosrv2':
        meta.update(upsampler=kw['upsampler'], upscale=kw['scale'], mid_dim=kw.get('mid_dim', 32))
    elif family == 'rgt':
        meta.update(split_size=kw['split_size'], num_heads=kw['num_heads'])
    elif family == 'atd':  # (atd_oracle.hyper_of(model) gives the same; this one needs no model)
        meta['hyper'] = dict(window_size=kw['window_size'], category_size=None, upscale=kw['upscale'], upsampler=kw['upsampler'], img_range=1.0, norm=True)
    return meta


class Case(CommonCase):
    """A configuration of this sweep (sweep_common.Case with these families' configurations, bars and oracle arguments)."""

    configs = CONFIGS
    family_bar = FAMILY_BAR
    make_meta = staticmethod(_meta)

    def __init__(self, name, device=None, **over):
        super().__init__(name, device, **over)
        if self.family == 'mosrv2' and not self.kw['unshuffle_mod']:
            self.P = 0  # MoSRv2 pads to its unshuffle factor only


# ------------------------------------------------------------------------------------------------------------ 1. consecutive sizes
@pytest.mark.parametrize('axis', ['h', 'w'])
@pytest.mark.parametrize('name', ALL)
def test_consecutive_sizes(device, name, axis):
    c = Case(name, device)
    sides = c.legal(axis)
    assert sides and sides == list(range(sides[0], c.tops[axis] + 1)) and c.accepts(c.other, c.other)
    assert not c.P or {(-s) % c.P for s in sides} == set(range(c.P))  # every pad from none to the largest is among them
    for i, s in enumerate(sides):
        x = _input(c, (2 if i == 0 else 1, c.cin, *c.hw(axis, s)), seed=100 * s + (axis == 'w'))
        _check(c, x, device, precision=('auto', 'bf16x3')[i % 2], what=f'size {axis}')


# ------------------------------------------------------------------------------------------------------------------ 2. acceptance
@pytest.mark.parametrize('name', ALL)
def test_engine_refuses_exactly_what_the_oracle_refuses(device, name):
    acceptance(Case(name, device), device)


# the configurations the README lists as refused: what the reference itself cannot build or run, and the heads that are not built
UNBUILT = [('smosr', dict(upsampler='conv', scale=2)), ('smosr', dict(upsampler='dysample', rep=True)), ('gfisrv2', dict(upsampler='transpose+conv')),
           ('gfisrv2', dict(upsampler='lda')), ('gfisrv2', dict(upsampler='pa_up', scale=4))]  # fmt: skip


@pytest.mark.parametrize('name,over', UNBUILT, ids=[f'{n}-' + '-'.join(str(v) for v in o.values()) for n, o in UNBUILT])
def test_unbuilt_configurations_are_refused_before_any_launch(device, name, over):
    lib = L.load()
    torch.cuda.synchronize()
    # Neither synthesiser makes such a checkpoint (SMoSR's builds the engine's module and is refused itself), so a legal one is re-labelled
    # in its MetaUpsample buffer, which is where the loader reads the head, the scale and ``rep`` from: the checkpoint path refuses.
    if name == 'gfisrv2':  # (from scale 2 up: at x1 every head is the one convolution)
        sd, key = dict(Case(name, scale=over.get('scale', 2)).sd), 'upscale.MetaUpsample'
        field = {1: SAMPLE_MODS3.index(over['upsampler'])}
    elif over['upsampler'] == 'conv':
        sd, key = dict(Case(name, scale=over['scale']).sd), 'upsampler.MetaUpsample'  # pixelshuffledirect at x2, called a conv head
        field = {1: SMOSR_MODS.index('conv')}
    else:
        sd, key = dict(Case(name, upsampler='dysample').sd), 'upsampler.MetaUpsample'  # a rep = 0 dysample checkpoint, called rep = 1
        field = {7: 1}
    assert isinstance(resselt_amd.load_from_state_dict(dict(sd)), torch.nn.Module)  # legal as synthesised
    sd[key] = sd[key].clone()
    for i, v in field.items():
        sd[key][i] = v
    with pytest.raises(NotImplementedError):
        m = resselt_amd.load_from_state_dict(sd).to(device)
        m(synth.synth_input((1, 3, 8, 9), seed=1).to(device))
    torch.cuda.synchronize()
    assert lib.rsa_check_status() == 0, f'{name} {over}: refused after a launch: {lib.rsa_last_error_string()}'


def test_gfisrv2_refuses_a_single_pixel(device):
    """1 x 1 is the one size the reference refuses (its view_as_complex raises: recorded in tests/golden/gfisrv2_tiny_probe.npz; the oracle's
    dense DFT has no such step, so the record decides here); 1 x 2 and 2 x 1 run, and right."""
    c = Case('gfisrv2', device)
    lib = L.load()
    probe = {tuple(p['size']): p['raises'] for p in load_golden('gfisrv2_tiny_probe')[0]['probe']}
    assert probe[1, 1] == 'RuntimeError' and probe[1, 2] is None and probe[2, 1] is None and c.accepts(1, 2) and c.accepts(2, 1)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        c.run(synth.synth_input((1, c.cin, 1, 1), seed=1).to(device))
    torch.cuda.synchronize()
    assert lib.rsa_check_status() == 0, f'refused after a launch: {lib.rsa_last_error_string()}'
    for hw in ((1, 2), (2, 1)):
        _check(c, _input(c, (1, c.cin, *hw), seed=8), device, what='beside the refused 1 x 1')


# ------------------------------------------------------------------------------------------------------------- 3. batch isolation
@pytest.mark.parametrize('name', ['rcan48', 'rcan64_unshuffle', 'eimn', 'fdat', 'fdat_unshuffle', 'omnisr_w4', 'omnisr_w8', 'gater', 'rgt', 'atd',
                                  'rha', 'rha_p16', 'flexnet', 'moesr', 'smosr', 'gfisrv2'])  # fmt: skip
def test_batch_of_three_different_images(device, name):
    """Whole-image reductions (channel attention means, ESA, latent attention, RG-SA's pooled keys, ATD's categories, GFISRv2's transforms),
    the cyclic roll and the window index must stay inside one image."""
    batch_of_three(Case(name, device), device, ['bf16x3'])


# ---------------------------------------------------------------------------------------------------------------- 4. heads against pads
HEADS = [
    ('mosr', dict(upsampler='ps', upscale=2)), ('mosr', dict(upsampler='ps', upscale=4)), ('mosr', dict(upsampler='dys', upscale=2)),
    ('mosr', dict(upsampler='dys', upscale=4)), ('mosr', dict(upsampler='gps', upscale=3)), ('mosr', dict(upsampler='gps', upscale=2)),
    # MoSRv2 pads only with unshuffle_mod: scale 1 unshuffles by 4 (pads up to 3), scale 2 by 2; the head then runs at x4
    ('mosrv2_u4', dict(upsampler='pixelshuffledirect')), ('mosrv2_u4', dict(upsampler='pixelshuffle')), ('mosrv2_u4', dict(upsampler='nearest+conv')),
    ('mosrv2_u4', dict(upsampler='dysample', mid_dim=16)), ('mosrv2_u2', dict(upsampler='pixelshuffle')), ('mosrv2_u2', dict(upsampler='nearest+conv')),
    ('mosrv2_u2', dict(upsampler='dysample', mid_dim=16)), ('mosrv2_u2', dict(upsampler='conv', scale=1, unshuffle_mod=False)),
    ('rha', dict(upsample='conv', scale=1)), ('rha', dict(upsample='pixelshuffledirect', scale=2)), ('rha', dict(upsample='pixelshuffledirect', scale=3)),
    ('rha', dict(upsample='pixelshuffle', scale=4)), ('rha', dict(upsample='pixelshuffle', scale=3)), ('rha', dict(upsample='nearest+conv', scale=2)),
    ('rha', dict(upsample='nearest+conv', scale=4)), ('rha', dict(upsample='dysample', scale=3)), ('rha', dict(upsample='dysample', scale=2)),
    ('fdat', dict(upsampler_type='conv', scale=1)), ('fdat', dict(upsampler_type='pixelshuffledirect', scale=3)), ('fdat', dict(upsampler_type='pixelshuffle', scale=4)),
    ('fdat', dict(upsampler_type='pixelshuffle', scale=2)), ('fdat', dict(upsampler_type='nearest+conv', scale=2)), ('fdat', dict(upsampler_type='nearest+conv', scale=3)),
    ('fdat', dict(upsampler_type='dysample', scale=2)), ('fdat', dict(upsampler_type='dysample', scale=4)), ('fdat', dict(upsampler_type='transpose+conv', scale=2)),
    ('fdat', dict(upsampler_type='transpose+conv', scale=3)), ('fdat', dict(upsampler_type='transpose+conv', scale=4)), ('fdat', dict(upsampler_type='lda', scale=2)),
    ('fdat', dict(upsampler_type='lda', scale=3)), ('fdat', dict(upsampler_type='pa_up', scale=2)), ('fdat', dict(upsampler_type='pa_up', scale=4)),
    ('fdat_unshuffle', dict(upsampler_type='transpose+conv')),
    ('flexnet', dict(upsampler='ps', scale=2)), ('flexnet', dict(upsampler='ps', scale=4)), ('flexnet', dict(upsampler='dys', scale=3)),
    ('flexnet', dict(upsampler='dys', scale=2)), ('flexnet', dict(upsampler='n+c', scale=3)), ('flexnet', dict(upsampler='n+c', scale=4)),
    ('atd', dict(upsampler='', upscale=1)), ('atd', dict(upsampler='pixelshuffle', upscale=3)), ('atd', dict(upsampler='pixelshuffle', upscale=2)),
    ('atd', dict(upsampler='pixelshuffledirect', upscale=2)), ('atd', dict(upsampler='pixelshuffledirect', upscale=3)), ('atd', dict(upsampler='nearest+conv', upscale=4)),
    # MoESR's five UniUpsample heads (DySample takes the features themselves), SMoSR's six (DySample end kernels 1 and 3), GFISRv2's five
    ('moesr', dict(upsampler='conv', scale=1)), ('moesr', dict(upsampler='pixelshuffledirect', scale=2)), ('moesr', dict(upsampler='pixelshuffledirect', scale=3)),
    ('moesr', dict(upsampler='pixelshuffle', scale=2)), ('moesr', dict(upsampler='pixelshuffle', scale=3, upsample_dim=24)), ('moesr', dict(upsampler='nearest+conv', scale=2)),
    ('moesr', dict(upsampler='nearest+conv', scale=4)), ('moesr', dict(upsampler='dysample', scale=2)), ('moesr', dict(upsampler='dysample', scale=3)),
    ('smosr', dict(upsampler='conv', scale=1)), ('smosr', dict(upsampler='pixelshuffledirect', scale=2, rep=True)), ('smosr', dict(upsampler='pixelshuffledirect', scale=3)),
    ('smosr', dict(upsampler='pixelshuffle', scale=3, upsampler_mid_dim=16)), ('smosr', dict(upsampler='pixelshuffle', scale=4, upsampler_mid_dim=20)),
    ('smosr', dict(upsampler='nearest+conv', scale=2, rep=True)), ('smosr', dict(upsampler='nearest+conv', scale=4)),
    ('smosr', dict(upsampler='dysample', scale=2, d_kernel=1)), ('smosr', dict(upsampler='dysample', scale=2, d_kernel=3)), ('smosr', dict(upsampler='dysample', scale=3, d_kernel=3, upsampler_mid_dim=20)),
    ('smosr', dict(upsampler='pa_up', scale=3, upsampler_mid_dim=24)), ('smosr', dict(upsampler='pa_up', scale=4, rep=True)),
    ('gfisrv2', dict(upsampler='conv', scale=1)), ('gfisrv2', dict(upsampler='pixelshuffledirect', scale=2)), ('gfisrv2', dict(upsampler='pixelshuffledirect', scale=4)),
    ('gfisrv2', dict(upsampler='pixelshuffle', scale=2, mid_dim=24)), ('gfisrv2', dict(upsampler='pixelshuffle', scale=3, mid_dim=16)), ('gfisrv2', dict(upsampler='nearest+conv', scale=3)),
    ('gfisrv2', dict(upsampler='nearest+conv', scale=4)), ('gfisrv2', dict(upsampler='dysample', scale=2, mid_dim=16)), ('gfisrv2', dict(upsampler='dysample', scale=3)),
]  # fmt: skip


@pytest.mark.parametrize('name,over', HEADS, ids=[f'{n}-' + '-'.join(str(v) for v in o.values()) for n, o in HEADS])
def test_heads_at_the_largest_pad(device, name, over):
    """The crop after the head with the largest legal pad on one axis and a pad of 1 on the other, and transposed."""
    c = Case(name, device, **over)
    h, w = _largest_pad_and_pad_one(c)
    assert c.accepts(h, w) and c.accepts(w, h)
    for i, hw in enumerate([(h, w), (w, h)]):
        _check(c, _input(c, (1, c.cin, *hw), seed=11 + i), device, precision=('auto', 'bf16x3')[i], what='head')


# ------------------------------------------------------------------------------------------------ 5. plan cache and precision switch
@pytest.mark.parametrize('name', ALL)
def test_plan_cache_and_precision_switch(device, name):
    c = Case(name, device)
    sides = c.legal('h')
    a, b = _input(c, (1, c.cin, sides[0], c.other), seed=21), _input(c, (1, c.cin, c.other, sides[-1]), seed=22)
    one_product = [p for p in c.m.precisions if not p.endswith('x3')][0]
    ad, bd = a.to(device), b.to(device)
    if c.family == 'atd':  # along fixed permutations, so that the comparison is of the plans and not of near-ties
        _check(c, a, device, precision='bf16x3', what='plan A')
        c.m.atd_record = False
        perms = {}
        for t in (ad, bd):
            c.m.atd_force, c.m.atd_record = None, True
            c.m(t)
            perms[t] = [p.clone() for _, p in c.m.atd_recorded]
        c.m.atd_record = False
    else:
        perms = None
        _check(c, a, device, precision='bf16x3', what='plan A')

    def run(t, precision):
        c.m.precision = precision
        if perms is not None:
            c.m.atd_force = perms[t]
        return c.m(t).clone()

    y1 = run(ad, 'bf16x3')
    yb = run(bd, 'bf16x3')
    assert torch.equal(run(ad, 'bf16x3'), y1), f'{name}: A after B differs from A'
    assert torch.equal(run(bd, 'bf16x3'), yb), f'{name}: B after A differs from B'
    y_one = run(ad, one_product)
    assert y_one.shape == y1.shape and torch.isfinite(y_one).all()
    assert torch.equal(run(ad, 'bf16x3'), y1), f"{name}: 'bf16x3' after {one_product!r} differs from the first run"
    assert torch.equal(run(ad, 'auto'), y1)


# ------------------------------------------------------------------------------------------------------------- 6. a multi-tile frame
@pytest.mark.parametrize('name', ONE_PER_FAMILY)
def test_multi_tile_frame(device, name):
    """70 x 150: ragged against every pad multiple here (2, 4, 8) and against the convolution tiles; several workgroups per kernel.  The
    float64 oracles take 0.2 s at the most at this size.  ATD: 21,888 category decisions, too many for all to be clear of a near-tie, so
    the input is taken as it comes and the 0.2 % cap of test_atd_gpu.py applies (between the float32 and the float64 run of the oracle on
    this input no decision differs)."""
    c = Case(name, device)
    x = _input(c, (1, c.cin, 70, 150), seed=31, guarded=False)
    _check(c, x, device, precision='bf16x3', atd_cap=0.002, what='multi-tile')


# ------------------------------------------------------------------------------------------------------- 7. tensor dtypes and layouts
@pytest.mark.parametrize('name', ONE_PER_FAMILY)
def test_tensor_dtypes_and_layouts(device, name):
    dtypes_and_layouts(Case(name, device), device, ['auto'], 'bf16x3')

