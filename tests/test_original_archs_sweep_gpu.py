"""RRDBNet, SPAN, SPANPlus, SpanPP, Compact, RTMoSR, SwinIR, DAT, HAT and DRCT on the GPU against their float64 CPU oracles (oracle/<arch>.py
through helpers.oracle_forward) at the shapes their fixtures do not reach, on the machinery of tests/sweep_common.py (``Case``,
``_images``, ``_input``, ``_where``, ``_check``: every case runs twice, the second run bit-equal).  For most of these families 'auto' is not
'bf16x3' but a one-product policy ('mixed', 'fp16') that takes other kernels throughout, so:

A. every 'auto' case asserts ``resolved_precision() == auto_precision`` before and after and runs with warnings turned into errors (an
   fp16-range fallback fails the case instead of testing 'bf16x3' twice); what 'auto' is per configuration is asserted on the CPU;
B. consecutive sizes: every legal height from the smallest through 18 at width 11 and every legal width through 34 at height 11 -- both
   edges of the 16 x 32 convolution tile crossed by one pixel either way, every pad from none to P - 1 -- each in 'auto' AND 'bf16x3';
C. acceptance: over the same ranges the engine raises exactly where the oracle raises, before any launch;
D. a batch of three images of different statistics at a size odd in both axes, per-image errors, both precisions (DRCT included: its plan
   repeats a per-image launch list over shared intermediates);
E. the variants of every family at the largest legal pad in H and a pad of 1 in W, and transposed;
F. plan cache (A, B, A again) and precision switch (every other mode of the family and back): bit-equal;
G. frames: 70 x 150 per family in both precisions; RRDBNet x4 also in three row bands (tail_band_rows = 24, the last one ragged) against the
   oracle; RRDBNet x2 and SPANPlus also one frame of more LR tiles than the device has CUs (269 x 507 = 272 tiles on 256 CUs: a persistent
   ring workgroup runs a second tile), in 'auto', against the float32 oracle;
H. fp16 / bf16 tensors, permuted and channels_last views (the same bits, the input untouched), and for RRDBNet uint8 images: every output
   code within 0.5 + 255 * tol of 255 * clamp(ref, 0, 1), the rule of test_conv_epilogue_matrix_gpu.py, tol the float32 bar of the case.

Tolerance (asserted): that of tests/fuzz_parity.py (``FUZZ_BAR`` of the newer sweep), in both precisions.  Each float32 case also prints
``err / family bar``, the bar being the family's own test file's (test_rrdbnet_gpu.TOL, test_span_gpu._tol, MODEL_REL of the SwinIR, DAT, HAT
and DRCT files); it is not asserted.

Worst err / tol and err / family bar per family, measured on an MI355X (profiles/original_archs_sweep_measure.txt has every MEASURE line):
RRDBNet 0.02 / 0.01, SPAN 0.27 / 0.07, SPANPlus 0.04 / 0.02, SpanPP 0.25 / 0.37, Compact 0.23 / 0.32, RTMoSR 0.21 / 0.05, SwinIR 0.58 / 0.58,
DAT 0.16 / 0.07, HAT 0.16 / 0.12, DRCT 0.16 / 0.12.  The worst err / tol is a bf16-tensor case except for SpanPP (70 x 150, 'mixed') and SwinIR
(8 x 11, 'mixed': one window row, pad 0).  No case exceeds its family bar.

What the sweep found: the engine ran HAT at heights of 5 to 8 (one row of windows), which the oracle refused -- the oracle's fault (a
strided view where the reference copies), fixed in oracle/hat.py and pinned by two new reference fixtures (5 x 11, 11 x 5).  ESRGAN+ listed
'mixed' among its modes but has no 'mixed' plan (it raised at pack time): the model no longer offers the mode.  RRDBNet's tail_band_rows,
set after a forward, had no effect on the plans already cached: setting it now drops them.
"""

import contextlib
import warnings

import pytest
import torch

from test_dat_gpu import MODEL_REL as DAT_REL
from test_drct_gpu import MODEL_REL as DRCT_REL
from test_hat_gpu import MODEL_REL as HAT_REL
from sweep_common import (FUZZ_BAR, Case, _check, _input, _largest_pad_and_pad_one, _state_dict, _status_ok, acceptance, batch_of_three,  # noqa: F401  (_status_ok: autouse)
                          dtypes_and_layouts)  # fmt: skip
from test_rrdbnet_gpu import TOL as RRDBNET_TOL
from test_span_gpu import _tol as span_bar
from test_swinir_gpu import MODEL_REL as SWINIR_REL

gpu = pytest.mark.gpu


def _rel(rel):
    return lambda ref: rel * max(1.0, ref.abs().max().item())


ORIGINAL_BAR = {'esrgan': lambda ref: RRDBNET_TOL['auto'], 'span': span_bar, 'spanplus': span_bar, 'spanpp': span_bar, 'compact': span_bar, 'rtmosr': span_bar,
                'swinir': _rel(SWINIR_REL), 'dat': _rel(DAT_REL), 'hat': _rel(HAT_REL), 'drct': _rel(DRCT_REL)}  # fmt: skip
SYNTH = {'esrgan': 'rrdbnet_state_dict'}

# name -> (family, synth keywords, pad multiple P, (top of the swept heights, of the swept widths), the other side: legal, of another residue)
TOPS = (18, 34)
ORIGINAL_CONFIGS = {
    'esrgan_x4': ('esrgan', dict(nb=1, scale=4), 0, TOPS, 11),
    'esrgan_x2': ('esrgan', dict(nb=2, scale=2), 0, TOPS, 11),
    'esrgan_unshuffle2': ('esrgan', dict(nb=1, scale=4, in_nc=12), 2, TOPS, 11),
    'esrgan_unshuffle4': ('esrgan', dict(nb=1, scale=4, in_nc=48), 4, TOPS, 11),
    'esrgan_plus': ('esrgan', dict(nb=1, scale=4, plus=True), 0, TOPS, 11),
    'span': ('span', dict(upscale=2), 0, TOPS, 11),
    'spanplus_ps': ('spanplus', dict(upscale=2, blocks=(2,), upsampler='ps'), 0, TOPS, 11),
    'spanplus_dys': ('spanplus', dict(upscale=2, blocks=(2,), upsampler='dys'), 0, TOPS, 11),
    'spanpp': ('spanpp', dict(feature_channels=32, implicit_dim=32, latent_layers=2), 0, TOPS, 11),
    'compact': ('compact', dict(num_feat=32, num_conv=2, upscale=2), 0, TOPS, 11),
    'rtmosr': ('rtmosr', dict(scale=2, dim=32, n_blocks=2), 2, TOPS, 11),
    'rtmosr_unshuffle': ('rtmosr', dict(scale=2, dim=32, n_blocks=2, unshuffle_mod=True), 4, TOPS, 11),
    'swinir_w8': ('swinir', dict(embed_dim=60, depths=(2,), num_heads=(6,), upscale=2, upsampler='pixelshuffledirect'), 8, TOPS, 11),
    'swinir_w7_gray': ('swinir', dict(in_ch=1, embed_dim=60, depths=(2,), num_heads=(6,), upscale=1, upsampler='', window=7, img_size=126), 7, TOPS, 11),
    'dat': ('dat', dict(embed_dim=64, depth=(2,), num_heads=(4,), split_size=(4, 8), upscale=2, img_size=16), 8, TOPS, 11),
    'hat': ('hat', dict(embed_dim=60, depths=(2,), num_heads=(6,), window=8, upscale=2), 8, TOPS, 11),
    'drct': ('drct', dict(embed_dim=60, gc=16, window=8, num_layers=1, upscale=2), 8, TOPS, 11),
}  # fmt: skip
ALL = list(ORIGINAL_CONFIGS)
ONE_PER_FAMILY = ['esrgan_x4', 'span', 'spanplus_ps', 'spanpp', 'compact', 'rtmosr', 'swinir_w8', 'dat', 'hat', 'drct']
# the smallest legal side at width 11, and what 'auto' resolves to
SMALLEST = dict(esrgan_x4=1, esrgan_x2=1, esrgan_unshuffle2=2, esrgan_unshuffle4=3, esrgan_plus=1, span=1, spanplus_ps=1, spanplus_dys=1, spanpp=1, compact=1,
                rtmosr=2, rtmosr_unshuffle=3, swinir_w8=5, swinir_w7_gray=4, dat=1, hat=5, drct=5)  # fmt: skip
AUTO = dict(esrgan_x4='mixed', esrgan_x2='mixed', esrgan_unshuffle2='mixed', esrgan_unshuffle4='mixed', esrgan_plus='bf16x3', span='bf16x3', spanplus_ps='mixed',
            spanplus_dys='mixed', spanpp='mixed', compact='fp16', rtmosr='bf16x3', rtmosr_unshuffle='bf16x3', swinir_w8='mixed', swinir_w7_gray='mixed', dat='mixed',
            hat='mixed', drct='mixed')  # fmt: skip
ONE_PRODUCT = ('mixed', 'fp16')


class OriginalCase(Case):
    """A configuration of the ten original families.  ``head_scale`` (SpanPP) is no synth keyword: it picks the head at the call.
    ``new_arch`` (RRDBNet) spells the same weights with the official Real-ESRGAN keys: the engine loads those, the oracle reads the old ones."""

    configs = ORIGINAL_CONFIGS
    family_bar = ORIGINAL_BAR

    @staticmethod
    def synth_name(family):
        return SYNTH.get(family, f'{family}_state_dict')

    @staticmethod
    def make_meta(family, kw):
        return dict(arch=family)

    def __init__(self, name, device=None, head_scale=None, new_arch=False, **over):
        self.head_scale, self.new_arch = head_scale, new_arch
        self.base = name
        super().__init__(name, device, **over)
        if head_scale is not None:
            self.name += f' head_scale={head_scale}'
            self.meta['scale'] = head_scale
        if new_arch:
            self.name += ' new_arch'
        # the window pads follow the variant: DAT pads to its larger split, the Swin families to their window
        if 'split_size' in over:
            self.P = max(over['split_size'])
        if 'window' in over:
            self.P = over['window']

    def engine_sd(self):
        if not self.new_arch:
            return self.sd
        sd = _state_dict(self.synth_name(self.family), tuple(sorted(dict(self.kw, new_arch=True).items())))
        assert set(sd) != set(self.sd) and all(any(torch.equal(v, t) for t in sd.values() if t.shape == v.shape) for v in self.sd.values())
        return sd

    def loaded(self):
        assert self.m.precision == 'auto' and self.m.parameters_info.in_channels == self.cin
        if not (set(self.kw) - set(self.configs[self.base][1])):  # (a variant may resolve otherwise: 'plus', an MLP the fused kernel does not take)
            assert self.m.auto_precision == AUTO[self.base]
        self.auto = self.m.auto_precision

    def run(self, x):
        return self.m(x) if self.head_scale is None else self.m(x, self.head_scale)

    @contextlib.contextmanager
    def running(self, precision):
        if precision != 'auto':
            yield
            return
        assert self.m.resolved_precision() == self.m.auto_precision == self.auto, f'{self.name}: auto is {self.m.resolved_precision()} before the run'
        with warnings.catch_warnings():
            warnings.simplefilter('error')  # the fp16-range fallback says so in a RuntimeWarning
            yield
        assert self.m.resolved_precision() == self.m.auto_precision == self.auto, f'{self.name}: auto is {self.m.resolved_precision()} after the run'

    def label(self, precision):
        return f'auto={self.auto}' if precision == 'auto' else precision


# ----------------------------------------------------------------------------------------------------------- A. what 'auto' is (CPU)
@pytest.mark.parametrize('name', ALL)
def test_auto_precision_of_every_configuration(name):
    import resselt_amd

    c = OriginalCase(name)
    m = resselt_amd.load_from_state_dict(dict(c.sd))
    assert m.precision == 'auto' and m.auto_precision == m.resolved_precision() == AUTO[name] and AUTO[name] in m.precisions
    if c.kw.get('plus'):  # ESRGAN+ has no 'mixed' plan and does not offer the mode
        m.precision = 'mixed'
        with pytest.raises(ValueError):
            m.resolved_precision()
    needs_one_product = c.family in ('spanplus', 'spanpp', 'compact', 'dat', 'hat', 'drct') or (c.family == 'esrgan' and not c.kw.get('plus'))
    if needs_one_product or c.family == 'swinir':  # (both SwinIR configurations are ones its property gives the fused whole-block kernel)
        assert m.auto_precision in ONE_PRODUCT, f'{name}: auto is {m.auto_precision}'


# ------------------------------------------------------------------------------------------------------------ B. consecutive sizes
@gpu
@pytest.mark.parametrize('axis', ['h', 'w'])
@pytest.mark.parametrize('name', ALL)
def test_consecutive_sizes_in_both_precisions(device, name, axis):
    c = OriginalCase(name, device)
    sides = c.legal(axis)
    assert sides and sides == list(range(sides[0], c.tops[axis] + 1)) and c.accepts(c.other, c.other)  # one contiguous range
    assert sides[0] == SMALLEST[name]
    assert not c.P or {(-s) % c.P for s in sides} == set(range(c.P))  # every pad from none to the largest is among them
    assert {15, 16, 17} <= set(c.legal('h')) and {31, 32, 33} <= set(c.legal('w')) and 2 * c.P + 1 <= 17  # both tile edges, one pixel either way
    xs = {s: _input(c, (2 if i == 0 else 1, c.cin, *c.hw(axis, s)), seed=100 * s + (axis == 'w')) for i, s in enumerate(sides)}
    refs = {}
    for precision in ('auto', 'bf16x3'):  # (one after the other: a switch repacks the weights)
        for s in sides:
            _, refs[s] = _check(c, xs[s], device, precision=precision, what=f'size {axis}', ref=refs.get(s))


# ------------------------------------------------------------------------------------------------------------------ C. acceptance
@gpu
@pytest.mark.parametrize('name', ALL)
def test_engine_refuses_exactly_what_the_oracle_refuses(device, name):
    acceptance(OriginalCase(name, device), device)


# ------------------------------------------------------------------------------------------------------------- D. batch isolation
@gpu
@pytest.mark.parametrize('name', ALL)
def test_batch_of_three_different_images(device, name):
    batch_of_three(OriginalCase(name, device), device, ['auto', 'bf16x3'])


# ------------------------------------------------------------------------------------------------------------------- E. variants
VARIANTS = [
    ('esrgan_x4', dict(scale=1)), ('esrgan_x4', dict(scale=2)), ('esrgan_x4', dict(scale=4)), ('esrgan_x4', dict(scale=8)), ('esrgan_x4', dict(new_arch=True)),
    ('esrgan_x2', dict(new_arch=True)),
    ('span', dict(upscale=2)), ('span', dict(upscale=4)), ('span', dict(norm=False)),
    ('spanplus_ps', dict(upscale=2)), ('spanplus_ps', dict(upscale=3)), ('spanplus_ps', dict(upscale=4)), ('spanplus_dys', dict(upscale=2)),
    ('spanplus_dys', dict(upscale=3)), ('spanplus_dys', dict(upscale=4)), ('spanplus_ps', dict(blocks=(1, 1))), ('spanplus_dys', dict(blocks=(1, 1))),
    ('spanpp', dict(head_scale=1)), ('spanpp', dict(head_scale=2)), ('spanpp', dict(head_scale=3)), ('spanpp', dict(head_scale=4)),
    ('compact', dict(upscale=2, num_feat=32)), ('compact', dict(upscale=4, num_feat=32)), ('compact', dict(upscale=2, num_feat=64)), ('compact', dict(upscale=4, num_feat=64)),
    ('rtmosr', dict(se=True, dccm=True)), ('rtmosr', dict(se=False, dccm=True)), ('rtmosr', dict(se=True, dccm=False)), ('rtmosr', dict(se=False, dccm=False)),
    ('rtmosr', dict(scale=4)), ('rtmosr_unshuffle', dict(se=False)),
    ('swinir_w8', dict(upsampler='', upscale=1)), ('swinir_w8', dict(upsampler='pixelshuffle')), ('swinir_w8', dict(upsampler='pixelshuffledirect')),
    ('swinir_w8', dict(upsampler='nearest+conv', upscale=4)), ('swinir_w8', dict(resi='3conv')), ('swinir_w8', dict(mlp_ratio=2.0)), ('swinir_w8', dict(mlp_ratio=4.0)),
    ('dat', dict(split_size=(2, 4))), ('dat', dict(split_size=(4, 8))), ('dat', dict(split_size=(8, 8))), ('dat', dict(split_size=(2, 4), upscale=3)),
    ('dat', dict(split_size=(4, 8), upscale=3)), ('dat', dict(split_size=(8, 8), upscale=3)),
    ('hat', dict(window=4)), ('hat', dict(window=8)), ('hat', dict(window=4, upscale=4)), ('hat', dict(window=8, upscale=4)),
    ('drct', dict(window=4)), ('drct', dict(window=8)), ('drct', dict(mlp_ratio=2.0)), ('drct', dict(mlp_ratio=4.0)), ('drct', dict(num_layers=2)),
    ('drct', dict(attn_mask=False)),
]  # fmt: skip


@gpu
@pytest.mark.parametrize('name,over', VARIANTS, ids=[f'{n}-' + '-'.join(f'{k}={v}' for k, v in o.items()) for n, o in VARIANTS])
def test_variants_at_the_largest_pad(device, name, over):
    """The crop after the head with the largest legal pad on one axis and a pad of 1 on the other, and transposed."""
    c = OriginalCase(name, device, **over)
    h, w = _largest_pad_and_pad_one(c)
    assert c.accepts(h, w) and c.accepts(w, h)
    for i, hw in enumerate([(h, w), (w, h)]):
        _check(c, _input(c, (1, c.cin, *hw), seed=11 + i), device, precision=('auto', 'bf16x3')[i], what='variant')


# ------------------------------------------------------------------------------------------------ F. plan cache and precision switch
@gpu
@pytest.mark.parametrize('name', ALL)
def test_plan_cache_and_precision_switch(device, name):
    c = OriginalCase(name, device)
    sides = c.legal('h')
    a, b = _input(c, (1, c.cin, sides[0], c.other), seed=21), _input(c, (1, c.cin, c.other, c.legal('w')[-1]), seed=22)
    ad, bd = a.to(device), b.to(device)

    def run(t, precision):
        c.m.precision = precision
        with c.running(precision):
            y = c.run(t).clone()
            torch.cuda.synchronize()
        return y

    for first in ('auto', 'bf16x3'):
        _check(c, a, device, precision=first, what='plan A')
        y1 = run(ad, first)
        yb = run(bd, first)
        assert torch.equal(run(ad, first), y1), f'{name} {first}: A after B differs from A'
        assert torch.equal(run(bd, first), yb), f'{name} {first}: B after A differs from B'
        for other in c.m.precisions:  # every mode of the family, the first one's own name among them
            y_other = run(ad, other)
            assert y_other.shape == y1.shape and torch.isfinite(y_other).all(), f'{name}: {other}'
            if other == c.m.auto_precision and first == 'auto':
                assert torch.equal(y_other, y1), f"{name}: {other!r} by name differs from 'auto'"
            assert torch.equal(run(ad, first), y1), f'{name}: {first!r} after {other!r} differs from the first run'


# -------------------------------------------------------------------------------------------------------------------- G. frames
@gpu
@pytest.mark.parametrize('name', ONE_PER_FAMILY)
def test_multi_tile_frame(device, name):
    """70 x 150: ragged against every pad multiple here and against the convolution tiles; several workgroups per kernel."""
    c = OriginalCase(name, device)
    x, ref = _input(c, (1, c.cin, 70, 150), seed=31), None
    for precision in ('auto', 'bf16x3'):
        _, ref = _check(c, x, device, precision=precision, what='multi-tile', ref=ref)


@gpu
def test_rrdbnet_banded_tail_against_the_oracle(device):
    """tail_band_rows = 24 at 70 rows: bands of 24, 24 and 22 rows, each with its halo rows recomputed, in 'auto' (the path of the 1080p
    headline, which runs four bands) and in 'bf16x3'.  Against the oracle; the distance to a one-band model is printed.  A band adds the
    same launches whatever the precision, and setting tail_band_rows after a forward takes effect (the plans of the old value are dropped)."""
    c, one = OriginalCase('esrgan_x4', device), OriginalCase('esrgan_x4', device)
    c.m.tail_band_rows = 24  # before the first forward
    assert one.m.tail_band_rows >= 70
    x, ref = _input(c, (1, c.cin, 70, 150), seed=31), None
    xd = x.to(device)
    for precision in ('auto', 'bf16x3'):
        y, ref = _check(c, x, device, precision=precision, what='three bands', ref=ref)
        banded = c.m.launches_per_forward()
        one.m.precision = precision
        with one.running(precision):
            whole = one.run(xd)
            torch.cuda.synchronize()
        single = one.m.launches_per_forward()
        # per extra band: two upconvs, the HR conv and the last conv again; the last conv goes through a band buffer and a copy in every band
        assert banded > single, f'{precision}: {banded} launches with tail_band_rows = 24, {single} with one band -- the banded plan was not built'
        d = (y - whole.cpu().double()).abs().max().item()
        print(f'MEASURE esrgan [esrgan_x4] three bands ({banded} launches) against one band ({single}), {c.label(precision)}: max-abs {d:.3e} '
              f'(printed; each is held to the oracle)')  # fmt: skip
    # the attribute after a forward: the cached one-band plans go, the next forward runs three bands and gives the bits of the model above
    one.m.tail_band_rows = 24
    again = one.run(xd)
    torch.cuda.synchronize()
    assert one.m.launches_per_forward() == banded and torch.equal(again.cpu().double(), y)
    one.m.tail_band_rows = 272
    assert torch.equal(one.run(xd), whole) and one.m.launches_per_forward() == single


@gpu
@pytest.mark.parametrize('name', ['esrgan_x2', 'spanplus_ps'])
def test_more_tiles_than_compute_units(device, name):
    """The smallest frame at which a persistent ring workgroup runs a second 16 x 32 tile (the fused pair, the coded conv5 and the
    LDS-resident weights keep state across tiles): 16 tile columns, and the fewest tile rows that give more tiles than CUs.  The oracle
    runs in float32 at this size (a few seconds), as the PLKSR sweep's large frames do."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    k = cus // 16 + 1
    h, w = 16 * k - 3, 32 * 16 - 5
    assert 16 * k > cus >= 16 * (k - 1)
    c = OriginalCase(name, device)
    print(f'MEASURE {c.family} [{name}] more tiles than CUs: {k} x 16 = {16 * k} tiles of 16 x 32 on {cus} CUs, {h} x {w}')
    _check(c, _input(c, (1, c.cin, h, w), seed=33), device, precision='auto', f64=False, what='more tiles than CUs')


# ------------------------------------------------------------------------------------------- H. tensor dtypes, layouts, 8-bit images
@gpu
@pytest.mark.parametrize('name', ALL)
def test_tensor_dtypes_and_layouts(device, name):
    c = OriginalCase(name, device)
    dtypes_and_layouts(c, device, ['auto', 'bf16x3'], 'auto')
    assert c.m.resolved_precision() == c.auto


@gpu
@pytest.mark.parametrize('name', [n for n in ALL if ORIGINAL_CONFIGS[n][0] == 'esrgan'])
def test_uint8_images(device, name):
    """uint8 [N, H, W, C] in and out: /255 in the first layout kernel, clamp * 255 + round in the last convolution's store."""
    c = OriginalCase(name, device)
    assert c.m.supports_u8
    for i, (h, w) in enumerate([(SMALLEST[name], c.other), (17, 33), (16, 32)]):
        assert c.accepts(h, w)
        x = _input(c, (2 if i == 0 else 1, c.cin, h, w), seed=51 + i)
        u = (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        xf = u.permute(0, 3, 1, 2).float() / 255
        ref = c.oracle(xf)
        tol = FUZZ_BAR[torch.float32] * max(1.0, ref.abs().max().item())
        want = 255 * ref.clamp(0, 1).permute(0, 2, 3, 1)
        assert (want == 0).any() and (want > 1).float().mean() > 0.3  # the clamp at 0 and codes above it (these weights stay far below 255)
        ud = u.to(device)
        for precision in ('auto', 'bf16x3'):
            c.m.precision = precision
            with c.running(precision):
                y = c.run(ud)
                torch.cuda.synchronize()
                y2 = c.run(ud)
                torch.cuda.synchronize()
            assert y.dtype == torch.uint8 and y.shape == want.shape, f'{name}: {tuple(y.shape)} {y.dtype}'
            d = (y.cpu().double() - want).abs()
            print(f'MEASURE {c.family} [{name}] uint8 {tuple(u.shape)} {c.label(precision)}: worst code error {d.max().item():.4f} / {0.5 + 255 * tol:.4f}')
            assert d.max().item() <= 0.5 + 255 * tol, f'{name} {precision} {h} x {w}: a code is {d.max().item():.4f} from 255 * clamp(ref), at {torch.unravel_index(d.argmax(), d.shape)}'
            assert torch.equal(y2, y) and torch.equal(ud.cpu(), u)
