"""What the whole-model GPU sweeps share (test_newer_archs_sweep_gpu.py, test_original_archs_sweep_gpu.py): a configuration object
(``Case``), image-like inputs, the comparison with the float64 oracle (``_check``: every case runs twice, the second run bit-equal, a MEASURE
line per case, the place of the largest error on a failure) and the bodies of the tests both sweeps run on their own configurations.

Tolerance (asserted): ``FUZZ_BAR``, the numbers of tests/fuzz_parity.py; the family bar of a ``Case`` is printed beside it, not asserted.
"""

import contextlib
import functools

import pytest
import torch

import resselt_amd
from atd_trajectory import guarded_input, run_on_engine_trajectory
from helpers import oracle_forward
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

FUZZ_BAR = {torch.float32: 3e-4, torch.float16: 2e-3, torch.bfloat16: 1.2e-2}  # tests/fuzz_parity.py
SEED = 61


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


@functools.lru_cache(maxsize=None)
def _state_dict(synth_name, kw_items):
    return getattr(synth, synth_name)(seed=SEED, **dict(kw_items))


@functools.lru_cache(maxsize=None)
def _in_channels(synth_name, kw_items):
    """The channel count of the images the configuration takes (after any unshuffle: what the loader reports)."""
    return resselt_amd.load_from_state_dict(dict(_state_dict(synth_name, kw_items))).parameters_info.in_channels


class Case:
    """One configuration: its state dict (made once), what its oracle needs besides, and a model on the device.  Each sweep subclasses it
    with its own ``configs`` (name -> (family, synth keywords, pad multiple P, top of the swept range or (top of heights, top of widths),
    the other side)), ``family_bar`` (family -> bar(ref), printed) and ``make_meta``, and the hooks below."""

    configs: dict = {}
    family_bar: dict = {}

    @staticmethod
    def make_meta(family, kw):
        """What helpers.oracle_forward needs besides the state dict."""
        return dict(arch=family)

    @staticmethod
    def synth_name(family):
        return f'{family}_state_dict'

    def __init__(self, name, device=None, **over):
        self.family, kw, self.P, top, self.other = self.configs[name]
        self.tops = dict(zip('hw', top if isinstance(top, tuple) else (top, top)))  # the top of the swept range of heights, of widths
        self.top = max(self.tops.values())
        self.kw = dict(kw, **over)
        self.name = name + ''.join(f' {k}={v}' for k, v in over.items())
        self.key = (type(self), self.family, tuple(sorted(self.kw.items())))
        self.sd = _state_dict(self.synth_name(self.family), self.key[2])
        self.cin = _in_channels(self.synth_name(self.family), self.key[2])
        self.meta = self.make_meta(self.family, self.kw)
        self.m = None
        if device is not None:
            self.m = resselt_amd.load_from_state_dict(dict(self.engine_sd())).to(device)
            self.loaded()

    def engine_sd(self):
        """The state dict the engine loads: the oracle's, unless a variant is another spelling of the same weights."""
        return self.sd

    def loaded(self):
        assert self.m.resolved_precision() == 'bf16x3'

    def run(self, x):
        return self.m(x)

    def running(self, precision):
        """The context both forwards of a ``_check`` run in."""
        return contextlib.nullcontext()

    def label(self, precision):
        """How a MEASURE line names the precision."""
        return precision

    def oracle(self, x, f64=True):
        """The oracle on the float values of ``x``, in float64 (or float32), as float64."""
        dt = torch.float64 if f64 else torch.float32
        with torch.no_grad():
            sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in self.sd.items()}
            return oracle_forward(self.meta, sd, x.float().to(dt)).to(torch.float64)

    def accepts(self, h, w):
        """Whether the oracle runs an h x w input (it raises exactly where the reference does)."""
        return _accepts(*self.key, self.cin, h, w)

    def legal(self, axis):
        """Every side in 1..top (of that axis) the oracle accepts on ``axis`` beside ``other``."""
        return [s for s in range(1, self.tops[axis] + 1) if self.accepts(*self.hw(axis, s))]

    def hw(self, axis, s):
        return (s, self.other) if axis == 'h' else (self.other, s)


@functools.lru_cache(maxsize=None)
def _accepts(cls, family, kw_items, cin, h, w):
    try:
        with torch.no_grad():
            oracle_forward(cls.make_meta(family, dict(kw_items)), _state_dict(cls.synth_name(family), kw_items), synth.synth_input((1, cin, h, w), seed=1))
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


def _check(c, x, device, *, precision='auto', f64=True, atd_cap=0.0, what='', ref=None):
    """Run ``x`` (any dtype) twice on ``c.m``; compare the first output with the oracle on the same values (``ref``, where the caller has
    it already), the second with the first."""
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
        ref = c.oracle(x, f64) if ref is None else ref
        c.m.precision = precision
        xd = x.to(device)
        with c.running(precision):
            y = c.run(xd)
            torch.cuda.synchronize()
            y2 = c.run(xd)
            torch.cuda.synchronize()
    assert y.shape == ref.shape and y.dtype == x.dtype, f'{c.name} {what}: {tuple(y.shape)} {y.dtype} for {tuple(ref.shape)}'
    got = y.cpu().to(torch.float64)
    err = (got - ref).abs().max().item()
    tol = FUZZ_BAR[x.dtype] * max(1.0, ref.abs().max().item())
    fam = f'{err / c.family_bar[c.family](ref):.3f}' if x.dtype == torch.float32 else 'n/a'
    print(f'MEASURE {c.family} [{c.name}] {what} {tuple(x.shape)} {str(x.dtype)[6:]} {c.label(precision)}{"" if f64 else " (float32 oracle)"}: max-abs {err:.3e} / tol {tol:.3e} = {err / tol:.3f}; '
          f'err / family bar = {fam}')  # fmt: skip
    if not err <= tol:
        print(_where(got, ref, c.P, x.shape[2:]))
    assert err <= tol, f'{c.name} {what} {tuple(x.shape)}: max-abs {err:.3e} > {tol:.3e}; {_where(got, ref, c.P, x.shape[2:])}'
    assert torch.equal(y2, y), f'{c.name} {what}: the cached plan gave different bits'
    return got, ref


def _largest_pad_and_pad_one(c):
    """(h, w): h the legal side with the largest pad, w a legal side with a pad of 1 (without padding: the smallest side and an odd one)."""
    sides = c.legal('h')
    if not c.P:
        return sides[0], 7
    h = max(sides, key=lambda s: ((-s) % c.P, -s))
    w = [s for s in sides if (-s) % c.P == 1 % c.P][0]
    return h, w


def acceptance(c, device):
    lib = L.load()
    refused = 0
    for axis in 'hw':
        legal = set(c.legal(axis))
        for s in range(1, c.tops[axis] + 1):
            hw = c.hw(axis, s)
            x = synth.synth_input((1, c.cin, *hw), seed=s).to(device)
            torch.cuda.synchronize()
            if s in legal:
                y = c.run(x)  # must not raise
                assert y.shape[0] == 1 and y.shape[2] % hw[0] == 0 and y.shape[3] % hw[1] == 0, f'{c.name} {hw}'
            else:
                refused += 1
                with pytest.raises((RuntimeError, ValueError, NotImplementedError)):
                    c.run(x)
                torch.cuda.synchronize()
                assert lib.rsa_check_status() == 0, f'{c.name} {hw}: refused after a launch: {lib.rsa_last_error_string()}'
    print(f'MEASURE {c.family} [{c.name}] acceptance: {refused} of {sum(c.tops.values())} sizes refused by the oracle and by the engine')
    s = c.legal('h')[0]
    _check(c, _input(c, (1, c.cin, *c.hw('h', s)), seed=7), device, what='after the refusals')  # the module still works, and still right


def batch_of_three(c, device, precisions):
    h, w = [s for s in c.legal('h') if s % 2][-1], c.other | 1
    assert h % 2 and w % 2 and c.accepts(h, w)
    x = _input(c, (3, c.cin, h, w), seed=5)
    assert x[1].mean() > x[0].mean() + 0.2 and x[1].std() < 0.5 * x[0].std() and x[2].std() > 1.5 * x[0].std()
    ref = None
    for precision in precisions:
        y, ref = _check(c, x, device, precision=precision, what='batch of three', ref=ref)
        print(f'MEASURE {c.family} [{c.name}] batch of three {c.label(precision)}, error per image: '
              + ', '.join(f'{v:.2e}' for v in (y - ref).abs().flatten(1).max(1).values.tolist()))  # fmt: skip


def dtypes_and_layouts(c, device, half_precisions, layout_precision):
    h, w = [s for s in c.legal('h') if s % 2][-1], c.other
    for dt in (torch.float16, torch.bfloat16):
        x, ref = _input(c, (2, c.cin, h, w), seed=41, dt=dt).to(dt), None
        for precision in half_precisions:
            _, ref = _check(c, x, device, precision=precision, what='half tensors', ref=ref)
    x = _input(c, (2, c.cin, h, w), seed=41)
    c.m.precision = layout_precision
    xd = x.to(device)
    if c.family == 'atd':
        c.m.atd_record = True
        c.m(xd)
        c.m.atd_force, c.m.atd_record = [p.clone() for _, p in c.m.atd_recorded], False
    keep = xd.clone()
    y = c.run(xd).clone()
    views = {'permuted': xd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), 'channels_last': xd.contiguous(memory_format=torch.channels_last)}
    if c.cin == 1:
        del views['channels_last']  # (with one channel it is the contiguous layout)
    for what, v in views.items():
        assert not v.is_contiguous() and torch.equal(v, xd)
        v0 = v.clone()
        assert torch.equal(c.run(v), y), f'{c.name}: a {what} input gives other bits than its contiguous copy'
        assert torch.equal(v, v0) and v.stride() == v0.stride(), f'{c.name}: the {what} input was modified'
    assert torch.equal(xd, keep), f'{c.name}: the input was modified'
