"""rsa_layernorm, rsa_layernorm_gelu and rsa_rmsnorm through the C-ABI against f64, element by element, inside the forward-error bounds
derived in tests/norm_reference.py (tests/test_norm_reference.py shows on the CPU that those bounds catch a one-pass variance, a padded
channel count and a missing eps in exactly these cases).  Inputs, references and bounds come from that module's case list.

Every launch writes at plane offset 1 of a buffer with two planes more than it needs, filled with 3.0 (hi and lo): the plane before, the
plane after, any padding of the plane stride and any gap of the batch stride must come back as 3.0.  The f32 map sits between two guard
zones.  The pad lanes of the INPUT map (channels C .. 4 ceil(C / 4) - 1) hold 1000.0, not zeros: a kernel that lets them into a sum fails.

rsa_layernorm's dispatch (csrc/swin.hip): C <= 256 layernorm_regs_kernel<8>, 257..384 layernorm_regs_kernel<12>, above layernorm_kernel<false>
with gamma / beta in LDS up to C = 1024 and read from global memory above.  The C sweep crosses each boundary; 65 tokens per image is one full
and one 1-token block.  725 x 725 at C = 8 is 8213 blocks against the grid cap of 8192: the only way into the regs kernels' grid-stride loop.

Not covered: layernorm_kernel<true> (dispatched only at H * W >= 2^27 tokens per image) and the grid-stride loop of layernorm_kernel<false>
(more than 8192 blocks at C > 384: about 800 MB of input).  Neither can be built at test size.
"""

import ctypes as C

import pytest
import torch

import norm_reference as R
from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.tensors import PF_BF16, PF_F16

pytestmark = pytest.mark.gpu

SENTINEL = 3.0
POISON = 1000.0
GUARD = 64  # floats on either side of the f32 map
E_ARG, E_ALIGN = -1, -3
DT = {PF_BF16: torch.bfloat16, PF_F16: torch.float16}
# which form of the normalise step rsa_layernorm's kernels compute (every one of them is centred: see layernorm_regs_kernel's comment)
LN_FORM = 'centred'


@pytest.fixture(autouse=True)
def _status_ok():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert L.load().rsa_check_status() == 0, L.load().rsa_last_error_string()


def _stream(device):
    return C.c_void_p(ops.current_stream_ptr(device))


def _x_map(x, device):
    """NCHW f32 -> the f32 NCHW4c map, pad lanes of the last group poisoned."""
    n, c, h, w = x.shape
    p4 = (c + 3) // 4
    xp = torch.full((n, p4 * 4, h, w), POISON, dtype=torch.float32, device=device)
    xp[:, :c] = x.to(device)
    return xp.reshape(n, p4, 4, h, w).permute(0, 1, 3, 4, 2).contiguous()


class Out:
    """Sentinel-filled output buffers of one launch and what came back in them."""

    def __init__(self, device, n, c, h, w, fmt, hi, lo, f32, stride_pad=0, gap_planes=0):
        self.n, self.c, self.h, self.w, self.fmt = n, c, h, w, fmt
        self.P, self.p4, self.hw = (c + 7) // 8, (c + 3) // 4, h * w
        self.plane_stride = self.hw + stride_pad
        self.planes_alloc = self.P + 2 + gap_planes
        self.batch_stride = self.planes_alloc * self.plane_stride
        mk = lambda: torch.full((n, self.planes_alloc, self.plane_stride, 8), SENTINEL, dtype=DT[fmt], device=device)  # noqa: E731
        self.hi = mk() if hi else None
        self.lo = mk() if lo else None
        self.f32 = torch.full((2 * GUARD + n * self.p4 * self.hw * 4,), SENTINEL, dtype=torch.float32, device=device) if f32 else None

    def ptr(self, t):
        return None if t is None else t.data_ptr() + self.plane_stride * 16  # plane offset 1

    def f32_ptr(self):
        return None if self.f32 is None else self.f32.data_ptr() + GUARD * 4

    def fill(self, lp):
        lp.out_hi, lp.out_lo, lp.out_plane_stride, lp.out_batch_stride = self.ptr(self.hi), self.ptr(self.lo), self.plane_stride, self.batch_stride
        lp.out_f32, lp.out_fmt = self.f32_ptr(), self.fmt

    def planes(self):
        """f64 NCHW [n, 8 P, h, w] of what the planes hold, after checking that everything around them is untouched."""
        val = None
        for t in (self.hi, self.lo):
            if t is None:
                continue
            keep = torch.ones(t.shape[:3], dtype=torch.bool, device=t.device)
            keep[:, 1 : 1 + self.P, : self.hw] = False
            assert bool((t[keep] == SENTINEL).all()), 'a plane outside the output, stride padding or a batch gap was written'
            v = t[:, 1 : 1 + self.P, : self.hw].double()
            val = v if val is None else val + v
        return val.reshape(self.n, self.P, self.h, self.w, 8).permute(0, 1, 4, 2, 3).reshape(self.n, self.P * 8, self.h, self.w)

    def map(self):
        """f64 NCHW [n, 4 p4, h, w] of the f32 map, after checking both guard zones."""
        assert bool((self.f32[:GUARD] == SENTINEL).all()) and bool((self.f32[-GUARD:] == SENTINEL).all()), 'the f32 map was overrun'
        m = self.f32[GUARD:-GUARD].reshape(self.n, self.p4, self.h, self.w, 4)
        return m.permute(0, 1, 4, 2, 3).reshape(self.n, self.p4 * 4, self.h, self.w).double()


def _launch(entry, device, d, case_c, shape, out):
    n, h, w = shape
    keep = [_x_map(d['x'], device), d['gamma'].to(device), d['beta'].to(device)]
    if entry == 'rsa_rmsnorm':
        rc = L.load().rsa_rmsnorm(keep[0].data_ptr(), n, h, w, case_c, d['eps'], keep[1].data_ptr(), keep[2].data_ptr(), out.ptr(out.hi), out.ptr(out.lo),
                                  out.plane_stride, out.batch_stride, _stream(device))  # fmt: skip
    else:
        lp = L.LayerNormParams()
        lp.batch, lp.H, lp.W, lp.C, lp.eps = n, h, w, case_c, d['eps']
        lp.x_f32, lp.gamma, lp.beta = (t.data_ptr() for t in keep)
        out.fill(lp)
        rc = getattr(L.load(), entry)(C.byref(lp), _stream(device))
    L.check(rc, entry)
    torch.cuda.synchronize()


ENTRY = {'ln': 'rsa_layernorm', 'gelu': 'rsa_layernorm_gelu', 'rms': 'rsa_rmsnorm'}


def _run(device, case, fmt=PF_BF16, hi=True, lo=True, f32=True, stride_pad=0, gap_planes=0, on_device=False):
    """Launch the case's kernel and hold every output it wrote to the bound.  Returns the worst error / bound and the f64 values held by the
    planes (or the map) on the case's C channels."""
    d = R.make_case(case)
    if on_device:
        d = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    ref, bound = R.reference(case, d, LN_FORM)
    out = Out(device, case.n, case.C, case.H, case.W, fmt, hi, lo, f32, stride_pad, gap_planes)
    _launch(ENTRY[case.op], device, d, case.C, (case.n, case.H, case.W), out)
    ref, bound = ref.to(device), bound.to(device)
    worst, got = 0.0, None
    for name, full, term in (('planes', out.planes() if hi else None, R.plane_term(ref, fmt, lo)), ('map', out.map() if f32 else None, 0.0)):
        if full is None:
            continue
        assert bool((full[:, case.C :] == 0).all()), f'{name}: channels beyond C are not exact zeros'
        got = full[:, : case.C]
        err = (got - ref).abs()
        lim = bound + term
        at = int((err / lim.clamp_min(1e-300)).argmax())
        ratio = float((err / lim.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        print(f'MEASURE {ENTRY[case.op]} {case.name} fmt={fmt} {name}{"" if name == "map" else "+lo" if lo else " hi only"}: worst error / bound {ratio:.3f} '
              f'(error {float(err.flatten()[at]):.3e}, bound {float(lim.flatten()[at]):.3e}), max error {float(err.max()):.3e}, bound max {float(lim.max()):.3e}, '
              f'|ref|max {float(ref.abs().max()):.3f}, offset/sigma {d["ratio"]:g}')  # fmt: skip
        assert not got.isnan().any() and bool((err <= lim).all()), f'{name}: outside the bound'
        for tok, what in ((d['const_tok'], 'constant'), (d['zero_tok'], 'all-zero')):
            if tok is not None and case.op != 'gelu' and not (case.op == 'rms' and what == 'constant'):
                b, y, x = tok
                want = d['beta'].to(device).double()  # both pixels come out as beta (offset), within the bound
                assert bool(((got[b, :, y, x] - want).abs() <= lim[b, :, y, x]).all()), f'{name}: the {what} pixel is not beta'
    return worst, got


# ------------------------------------------------------------------------------------------------------------------ rsa_layernorm
@pytest.mark.parametrize('case', R.SWEEP, ids=lambda c: c.name)
def test_layernorm_c_sweep(device, case):
    _run(device, case)


@pytest.mark.parametrize('case', R.GEOMETRY, ids=lambda c: c.name)
def test_layernorm_token_geometry(device, case):
    _run(device, case)


def test_layernorm_grid_stride_loop(device):
    """8213 blocks on a grid of 8192: blocks 8192 .. 8212 are second iterations, which reuse s_red and skip the gamma / beta staging."""
    assert (R.GRID.H * R.GRID.W + 63) // 64 > 8192
    _run(device, R.GRID, on_device=True)


@pytest.mark.parametrize('fmt', [PF_BF16, PF_F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('hi,lo,f32', [(True, True, False), (True, False, False), (False, False, True), (True, True, True)], ids=['hi+lo', 'hi', 'f32', 'all'])
@pytest.mark.parametrize('case', R.FORMS, ids=lambda c: c.name)
def test_layernorm_output_forms(device, case, hi, lo, f32, fmt):
    _run(device, case, fmt, hi, lo, f32)


@pytest.mark.parametrize('case', [R.GEOMETRY[3], R.GEOMETRY[8]], ids=lambda c: c.name)
@pytest.mark.parametrize('stride_pad,gap_planes', [(5, 0), (0, 3)], ids=['plane-stride', 'batch-gap'])
def test_layernorm_placement(device, case, stride_pad, gap_planes):
    """A plane stride of H W + 5 units, and a batch stride that leaves three planes between the images."""
    _run(device, case, stride_pad=stride_pad, gap_planes=gap_planes)


@pytest.mark.parametrize('case', R.CONDITIONING, ids=lambda c: c.name)
def test_layernorm_conditioning(device, case):
    _run(device, case)


def test_layernorm_three_brackets_on_one_input(device):
    """The same 180 channels through layernorm_regs_kernel<8> (C 180), <12> (C 300) and layernorm_kernel<false> (C 400)."""
    got = [_run(device, case, hi=False, lo=False)[1][:, :180] for case in R.BRACKETS]
    ref, bound = R.reference(R.BRACKETS[0], R.make_case(R.BRACKETS[0]), LN_FORM)
    for name, a, b in (('<8> vs <12>', 0, 1), ('<8> vs generic', 0, 2), ('<12> vs generic', 1, 2)):
        diff = (got[a] - got[b]).abs().cpu()
        print(f'MEASURE rsa_layernorm brackets {name}: max difference {float(diff.max()):.3e} ({float((diff / bound).max()):.3f} of the bound at C = 180)')
        # each kernel is inside its own bound (asserted in _run) on statistics that agree (tests/test_norm_reference.py); the bound grows with C, so
        # two of them are apart by no more than the bounds at C = 400 and C = 180 together, and the C = 400 bound is below 3 x the one at 180
        assert bool((diff <= 4 * bound).all()), name


def _ln_params(device, c=20, n=2, h=3, w=5):
    out = Out(device, n, c, h, w, PF_BF16, True, True, True)
    keep = [_x_map(torch.zeros((n, c, h, w)), device), torch.ones(c, device=device), torch.zeros(c, device=device), out]
    lp = L.LayerNormParams()
    lp.batch, lp.H, lp.W, lp.C, lp.eps = n, h, w, c, 1e-5
    lp.x_f32, lp.gamma, lp.beta = (t.data_ptr() for t in keep[:3])
    out.fill(lp)
    return lp, keep


def test_layernorm_error_codes(device):
    lib, s = L.load(), _stream(device)
    assert lib.rsa_layernorm(None, s) == E_ARG and b'layernorm: null params' in lib.rsa_last_error_string()
    lp, keep = _ln_params(device)
    assert lib.rsa_layernorm(C.byref(lp), s) == 0
    for field, value, code, text in [('C', 0, E_ARG, b'bad geometry'), ('C', -4, E_ARG, b'bad geometry'), ('x_f32', None, E_ARG, b'null pointer'),
                                     ('gamma', None, E_ARG, b'null pointer'), ('beta', None, E_ARG, b'null pointer'), ('out_fmt', 2, E_ARG, b'out_fmt'),
                                     ('out_fmt', -1, E_ARG, b'out_fmt'), ('reserved0', 1, E_ARG, b'out_fmt'),
                                     ('x_f32', lp.x_f32 + 4, E_ALIGN, b'16-byte aligned'), ('out_hi', lp.out_hi + 8, E_ALIGN, b'16-byte aligned'),
                                     ('out_lo', lp.out_lo + 2, E_ALIGN, b'16-byte aligned'), ('out_f32', lp.out_f32 + 4, E_ALIGN, b'16-byte aligned'),
                                     ('out_plane_stride', lp.H * lp.W - 1, E_ARG, b'out_plane_stride')]:  # fmt: skip
        old = getattr(lp, field)
        setattr(lp, field, value)
        assert lib.rsa_layernorm(C.byref(lp), s) == code, field
        msg = lib.rsa_last_error_string()
        assert b'layernorm' in msg and text in msg, (field, msg)
        setattr(lp, field, old)
    lp.out_hi, lp.out_lo, lp.out_f32 = None, None, None  # neither planes nor a map
    assert lib.rsa_layernorm(C.byref(lp), s) == E_ARG and b'null pointer' in lib.rsa_last_error_string()
    lp, keep = _ln_params(device)
    lp.out_hi, lp.out_lo, lp.out_plane_stride = None, None, 0  # the map alone: the plane stride is not looked at (the patch-embed norms)
    assert lib.rsa_layernorm(C.byref(lp), s) == 0
    torch.cuda.synchronize()
    assert bool((keep[3].hi == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ rsa_layernorm_gelu
@pytest.mark.parametrize('fmt,lo', [(PF_BF16, True), (PF_BF16, False), (PF_F16, True), (PF_F16, False)], ids=['bf16+lo', 'bf16', 'fp16+lo', 'fp16'])
@pytest.mark.parametrize('case', R.GELU, ids=lambda c: c.name)
def test_layernorm_gelu(device, case, fmt, lo):
    _run(device, case, fmt, True, lo, False)


def test_layernorm_gelu_error_codes(device):
    lib, s = L.load(), _stream(device)
    lp, keep = _ln_params(device)
    assert lib.rsa_layernorm_gelu(C.byref(lp), s) == E_ARG and b'layernorm_gelu' in lib.rsa_last_error_string()  # out_f32 is set
    lp.out_f32 = None
    assert lib.rsa_layernorm_gelu(C.byref(lp), s) == 0
    for eps in (0.0, -1e-5):
        lp.eps = eps
        assert lib.rsa_layernorm_gelu(C.byref(lp), s) == E_ARG and b'layernorm_gelu' in lib.rsa_last_error_string()
    lp.eps = 1e-5
    assert lib.rsa_layernorm_gelu(C.byref(lp), s) == 0


# ------------------------------------------------------------------------------------------------------------------ rsa_rmsnorm
@pytest.mark.parametrize('lo', [True, False], ids=['hi+lo', 'hi'])
@pytest.mark.parametrize('case', R.RMS, ids=lambda c: c.name)
def test_rmsnorm(device, case, lo):
    """The all-zero pixel must give `offset` (asserted in _run with the bound u |offset|), not NaN."""
    _run(device, case, PF_BF16, True, lo, False)


def test_rmsnorm_error_codes(device):
    lib, s = L.load(), _stream(device)
    lp, keep = _ln_params(device)
    args = lambda batch=2, x=lp.x_f32, c=20: (x, batch, 3, 5, c, 1e-6, lp.gamma, lp.beta, lp.out_hi, lp.out_lo, lp.out_plane_stride, lp.out_batch_stride, s)  # noqa: E731
    assert lib.rsa_rmsnorm(*args()) == 0
    assert lib.rsa_rmsnorm(*args(batch=65536)) == E_ARG and b'rmsnorm' in lib.rsa_last_error_string()
    assert lib.rsa_rmsnorm(*args(c=0)) == E_ARG
    assert lib.rsa_rmsnorm(*args(x=lp.x_f32 + 4)) == E_ALIGN and b'rmsnorm' in lib.rsa_last_error_string()
