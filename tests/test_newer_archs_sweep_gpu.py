"""MoSR, MoSRv2, RGT, FDAT, OmniSR, ATD, RCAN, GateR, EIMN, RHA and FlexNet on the GPU against their float64 CPU oracles
(tests/<arch>_oracle.py through helpers.oracle_forward) at the shapes their fixtures do not reach:

1. consecutive sizes: every side the oracle accepts from 1 up to ``top`` (2 P + 1 for a pad multiple P, 9 without padding, further where
   the smallest legal side lies above that) on either axis, the other side fixed at another residue -- every pad from none to the largest
   legal one, one window, two windows plus a row;
2. acceptance: over the same range the engine raises exactly where the oracle (whose behaviour is the reference's) raises, before any launch;
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
GateR 0.54, EIMN 0.40, RHA 0.71, FlexNet 0.57 (absolute bars at about twice a fixture's error).  No case exceeds its family bar.
"""

import functools

import pytest
import torch

import resselt_amd
from atd_trajectory import guarded_input, run_on_engine_trajectory
from helpers import oracle_forward
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth
from test_atd_gpu import _tol as atd_bar
from test_eimn_gpu import TOL_BF16X3 as EIMN_BAR
from test_fdat_gpu import _tol as fdat_bar
from test_flexnet_gpu import TOL_BF16X3 as FLEXNET_BAR
from test_gater_gpu import TOL_BF16X3 as GATER_BAR
from test_mosr_gpu import _tol as mosr_bar
from test_omnisr_gpu import _tol as omnisr_bar
from test_rcan_gpu import TOL_BF16X3 as RCAN_BAR
from test_rgt_gpu import _tol as rgt_bar
from test_rha_gpu import TOL_BF16X3 as RHA_BAR

pytestmark = pytest.mark.gpu

FUZZ_BAR = {torch.float32: 3e-4, torch.float16: 2e-3, torch.bfloat16: 1.2e-2}  # tests/fuzz_parity.py
FAMILY_BAR = {'mosr': mosr_bar, 'mosrv2': mosr_bar, 'rgt': rgt_bar, 'fdat': fdat_bar, 'omnisr': omnisr_bar, 'atd': atd_bar,
              'rcan': lambda ref: RCAN_BAR, 'gater': lambda ref: GATER_BAR, 'eimn': lambda ref: EIMN_BAR, 'rha': lambda ref: RHA_BAR,
              'flexnet': lambda ref: FLEXNET_BAR}  # fmt: skip


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


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
}  # fmt: skip
ALL = list(CONFIGS)
ONE_PER_FAMILY = ['mosr', 'mosrv2_u4', 'rgt', 'fdat_unshuffle', 'omnisr_w8', 'atd', 'rcan64_unshuffle', 'gater', 'eimn', 'rha', 'flexnet']
SEED = 61


@functools.lru_cache(maxsize=None)
def _state_dict(family, kw_items):
    return getattr(synth, f'{family}_state_dict')(seed=SEED, **dict(kw_items))


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


class Case:
    """One configuration: its state dict (made once), what its oracle needs besides, and a model on the device."""

    def __init__(self, name, device=None, **over):
        self.family, kw, self.P, self.top, self.other = CONFIGS[name]
        self.kw = dict(kw, **over)
        self.name = name + ''.join(f' {k}={v}' for k, v in over.items())
        self.sd = _state_dict(self.family, tuple(sorted(self.kw.items())))
        if self.family == 'mosrv2' and not self.kw['unshuffle_mod']:
            self.P = 0  # MoSRv2 pads to its unshuffle factor only
        self.meta = _meta(self.family, self.kw)
        self.m = None
        if device is not None:
            self.m = resselt_amd.load_from_state_dict(dict(self.sd)).to(device)
            assert self.m.resolved_precision() == 'bf16x3'

    def oracle(self, x, f64=True):
        """The oracle on the float values of ``x``, in float64 (or float32), as float64."""
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in self.sd.items()}
            return oracle_forward(self.meta, sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        """Whether the oracle runs an h x w input (it raises exactly where the reference does)."""
        return _accepts(self.family, tuple(sorted(self.kw.items())), h, w)

    def legal(self, axis):
        """Every side in 1..top the oracle accepts on ``axis`` beside ``other``."""
        return [s for s in range(1, self.top + 1) if self.accepts(*self.hw(axis, s))]

    def hw(self, axis, s):
        return (s, self.other) if axis == 'h' else (self.other, s)


@functools.lru_cache(maxsize=None)
def _accepts(family, kw_items, h, w):
    try:
        with torch.no_grad():
            oracle_forward(_meta(family, dict(kw_items)), _state_dict(family, kw_items), synth.synth_input((1, 3, h, w), seed=1))
    except Exception:  # whatever the plain-torch restatement trips over: a reflect pad wider than the image, an empty pooling window, log(0)
        return False
    return True


def _images(shape, seed):
    """Image-like inputs; in a batch the second and third image have other statistics (as in test_realplksr_heads)."""
    x = synth.synth_input(shape, seed=seed)
    if shape[0] > 1:
        x[1] = x[1] * 0.3 + 0.6
    if shape[0] > 2:
        x[2] = x[2] * 2.0 - 0.5
    return x


def _input(c, shape, seed, guarded=True, dt=torch.float32):
    """float32 values that ``dt`` holds exactly; for ATD the first seed on which the oracle takes no near-tie decision."""
    make = lambda shape, seed: _images(shape, seed).to(dt).float()  # noqa: E731
    if c.family == 'atd' and guarded:
        return guarded_input(c.sd, c.meta['hyper'], shape, seed, make)
    return make(shape, seed)


def _where(y, ref, P, in_hw):
    """The place of the largest error, and whether it lies in the last pad multiple of output rows / columns."""
    d = (y - ref).abs()
    per_image = ', '.join(f'{v:.2e}' for v in d.flatten(1).max(1).values.tolist())
    n, ch, r, col = (int(v) for v in torch.unravel_index(d.argmax(), d.shape))
    band = max(1, P) * max(1, ref.shape[2] // in_hw[0])  # the pad multiple in output pixels
    return (f'largest error at image {n} channel {ch} row {r} of {ref.shape[2]} column {col} of {ref.shape[3]} '
            f'(in the last {band} rows: {r >= ref.shape[2] - band}; in the last {band} columns: {col >= ref.shape[3] - band}); per image: {per_image}')  # fmt: skip


def _check(c, x, device, *, precision='auto', f64=True, atd_cap=0.0, what=''):
    """Run ``x`` (any dtype) twice on ``c.m``; compare the first output with the oracle on the same values, the second with the first."""
    if c.family == 'atd':
        y, y2, ref, differ, total = run_on_engine_trajectory(c.m, c.sd, x.float(), device, 'bf16x3' if precision == 'auto' else precision,
                                                             torch.float64 if f64 else torch.float32)  # fmt: skip
        if x.dtype != torch.float32:  # (the trajectory helper ran the float values; the tensor dtype is tested on the same trajectory below)
            c.m.atd_record = False
            c.m.atd_force = [p for _, p in c.m.atd_recorded]
            y = c.m(x.to(device))
            y2 = c.m(x.to(device))
            c.m.atd_force = None
        ref = ref.to(torch.float64)
        assert differ <= atd_cap * total, f'{c.name} {what} {tuple(x.shape)}: {differ} of {total} category decisions differ from the oracle'
    else:
        ref = c.oracle(x, f64)
        c.m.precision = precision
        xd = x.to(device)
        y = c.m(xd)
        torch.cuda.synchronize()
        y2 = c.m(xd)
    assert y.shape == ref.shape and y.dtype == x.dtype, f'{c.name} {what}: {tuple(y.shape)} {y.dtype} for {tuple(ref.shape)}'
    got = y.cpu().to(torch.float64)
    err = (got - ref).abs().max().item()
    tol = FUZZ_BAR[x.dtype] * max(1.0, ref.abs().max().item())
    fam = f'{err / FAMILY_BAR[c.family](ref):.3f}' if x.dtype == torch.float32 else 'n/a'
    print(f'MEASURE {c.family} [{c.name}] {what} {tuple(x.shape)} {str(x.dtype)[6:]} {precision}: max-abs {err:.3e} / tol {tol:.3e} = {err / tol:.3f}; '
          f'err / family bar = {fam}')  # fmt: skip
    if not err <= tol:
        print(_where(got, ref, c.P, x.shape[2:]))
    assert err <= tol, f'{c.name} {what} {tuple(x.shape)}: max-abs {err:.3e} > {tol:.3e}; {_where(got, ref, c.P, x.shape[2:])}'
    assert torch.equal(y2, y), f'{c.name} {what}: the cached plan gave different bits'
    return got, ref


# ------------------------------------------------------------------------------------------------------------ 1. consecutive sizes
@pytest.mark.parametrize('axis', ['h', 'w'])
@pytest.mark.parametrize('name', ALL)
def test_consecutive_sizes(device, name, axis):
    c = Case(name, device)
    sides = c.legal(axis)
    assert sides and sides == list(range(sides[0], c.top + 1)) and c.accepts(c.other, c.other)
    assert not c.P or {(-s) % c.P for s in sides} == set(range(c.P))  # every pad from none to the largest is among them
    for i, s in enumerate(sides):
        x = _input(c, (2 if i == 0 else 1, 3, *c.hw(axis, s)), seed=100 * s + (axis == 'w'))
        _check(c, x, device, precision=('auto', 'bf16x3')[i % 2], what=f'size {axis}')


# ------------------------------------------------------------------------------------------------------------------ 2. acceptance
@pytest.mark.parametrize('name', ALL)
def test_engine_refuses_exactly_what_the_oracle_refuses(device, name):
    c = Case(name, device)
    lib = L.load()
    refused = 0
    for axis in 'hw':
        legal = set(c.legal(axis))
        for s in range(1, c.top + 1):
            hw = c.hw(axis, s)
            x = synth.synth_input((1, 3, *hw), seed=s).to(device)
            torch.cuda.synchronize()
            if s in legal:
                y = c.m(x)  # must not raise
                assert y.shape[0] == 1 and y.shape[2] % hw[0] == 0 and y.shape[3] % hw[1] == 0, f'{name} {hw}'
            else:
                refused += 1
                with pytest.raises((RuntimeError, ValueError, NotImplementedError)):
                    c.m(x)
                torch.cuda.synchronize()
                assert lib.rsa_check_status() == 0, f'{name} {hw}: refused after a launch: {lib.rsa_last_error_string()}'
    print(f'MEASURE {c.family} [{name}] acceptance: {refused} of {2 * c.top} sizes refused by the oracle and by the engine')
    s = c.legal('h')[0]
    _check(c, _input(c, (1, 3, *c.hw('h', s)), seed=7), device, what='after the refusals')  # the module still works, and still right


# ------------------------------------------------------------------------------------------------------------- 3. batch isolation
@pytest.mark.parametrize('name', ['rcan48', 'rcan64_unshuffle', 'eimn', 'fdat', 'fdat_unshuffle', 'omnisr_w4', 'omnisr_w8', 'gater', 'rgt', 'atd',
                                  'rha', 'rha_p16', 'flexnet'])  # fmt: skip
def test_batch_of_three_different_images(device, name):
    """Whole-image reductions (channel attention means, ESA, latent attention, RG-SA's pooled keys, ATD's categories), the cyclic roll and
    the window index must stay inside one image."""
    c = Case(name, device)
    h, w = [s for s in c.legal('h') if s % 2][-1], c.other | 1
    assert h % 2 and w % 2 and c.accepts(h, w)
    x = _input(c, (3, 3, h, w), seed=5)
    assert x[1].mean() > x[0].mean() + 0.2 and x[1].std() < 0.5 * x[0].std() and x[2].std() > 1.5 * x[0].std()
    y, ref = _check(c, x, device, precision='bf16x3', what='batch of three')
    print(f'MEASURE {c.family} [{name}] batch of three, error per image: ' + ', '.join(f'{v:.2e}' for v in (y - ref).abs().flatten(1).max(1).values.tolist()))


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
]  # fmt: skip


def _largest_pad_and_pad_one(c):
    """(h, w): h the legal side with the largest pad, w a legal side with a pad of 1 (without padding: the smallest side and an odd one)."""
    sides = c.legal('h')
    if not c.P:
        return sides[0], 7
    h = max(sides, key=lambda s: ((-s) % c.P, -s))
    w = [s for s in sides if (-s) % c.P == 1 % c.P][0]
    return h, w


@pytest.mark.parametrize('name,over', HEADS, ids=[f'{n}-' + '-'.join(str(v) for v in o.values()) for n, o in HEADS])
def test_heads_at_the_largest_pad(device, name, over):
    """The crop after the head with the largest legal pad on one axis and a pad of 1 on the other, and transposed."""
    c = Case(name, device, **over)
    h, w = _largest_pad_and_pad_one(c)
    assert c.accepts(h, w) and c.accepts(w, h)
    for i, hw in enumerate([(h, w), (w, h)]):
        _check(c, _input(c, (1, 3, *hw), seed=11 + i), device, precision=('auto', 'bf16x3')[i], what='head')


# ------------------------------------------------------------------------------------------------ 5. plan cache and precision switch
@pytest.mark.parametrize('name', ALL)
def test_plan_cache_and_precision_switch(device, name):
    c = Case(name, device)
    sides = c.legal('h')
    a, b = _input(c, (1, 3, sides[0], c.other), seed=21), _input(c, (1, 3, c.other, sides[-1]), seed=22)
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
    x = _input(c, (1, 3, 70, 150), seed=31, guarded=False)
    _check(c, x, device, precision='bf16x3', atd_cap=0.002, what='multi-tile')


# ------------------------------------------------------------------------------------------------------- 7. tensor dtypes and layouts
@pytest.mark.parametrize('name', ONE_PER_FAMILY)
def test_tensor_dtypes_and_layouts(device, name):
    c = Case(name, device)
    h, w = [s for s in c.legal('h') if s % 2][-1], c.other
    for dt in (torch.float16, torch.bfloat16):
        _check(c, _input(c, (2, 3, h, w), seed=41, dt=dt).to(dt), device, what='half tensors')
    x = _input(c, (2, 3, h, w), seed=41)
    c.m.precision = 'bf16x3'
    xd = x.to(device)
    if c.family == 'atd':
        c.m.atd_record = True
        c.m(xd)
        c.m.atd_force, c.m.atd_record = [p.clone() for _, p in c.m.atd_recorded], False
    keep = xd.clone()
    y = c.m(xd).clone()
    views = {'permuted': xd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), 'channels_last': xd.contiguous(memory_format=torch.channels_last)}
    for what, v in views.items():
        assert not v.is_contiguous() and torch.equal(v, xd)
        v0 = v.clone()
        assert torch.equal(c.m(v), y), f'{name}: a {what} input gives other bits than its contiguous copy'
        assert torch.equal(v, v0) and v.stride() == v0.stride(), f'{name}: the {what} input was modified'
    assert torch.equal(xd, keep), f'{name}: the input was modified'
