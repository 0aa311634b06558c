"""ATD on the GPU against its CPU oracle along the ENGINE's trajectory (shared by test_atd_gpu.py and test_newer_archs_sweep_gpu.py).

ATD sorts its tokens by the category of a similarity arg-max, so two float implementations may legitimately take different permutations
at a near-tie, after which their outputs are not comparable.  The engine therefore runs free with recording on; the oracle then runs with
the engine's permutations forced and computes its own ids along that trajectory.  Checked here: the engine's permutation is exactly the
stable sort of its ids, and (in three bf16 products) every differing id decision has an oracle top-two margin below TAU.  The caller
asserts the output error and the share of differing decisions.
"""

import torch

import atd_oracle as O


def run_on_engine_trajectory(m, sd, x, device, precision, dtype=torch.float32):
    """Returns (y, y2, ref, differ, total): the engine's first and second output for ``x`` (any floating dtype, on the CPU) as they came
    (device tensors), the oracle's output in ``dtype`` for the same values along the first run's recorded permutations, and how many of
    the ``total`` id decisions of that run differ from the oracle's."""
    m.precision = precision
    m.atd_record = True
    xd = x.to(device)
    y = m(xd)
    torch.cuda.synchronize()
    rec_e = [(i.cpu().long(), p.cpu().long()) for i, p in m.atd_recorded]
    y2 = m(xd)  # the cached plan; it records again, which the caller need not look at
    torch.cuda.synchronize()
    rec = {}
    with torch.no_grad():
        ref = O.atd_forward({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, x.to(dtype), O.hyper_of(m),
                            force=[p for _, p in rec_e], record=rec)  # fmt: skip
    assert len(rec_e) == len(rec['ids'])
    differ = total = 0
    for li, (ids, perm) in enumerate(rec_e):
        assert torch.equal(perm, torch.sort(ids, dim=-1, stable=True).indices), f'layer {li}: the permutation is not the stable sort of the ids'
        d = ids != rec['ids'][li]
        differ += int(d.sum())
        total += ids.numel()
        if d.any() and precision == 'bf16x3':
            worst = rec['margin'][li][d].max().item()
            assert worst < O.TAU, f'layer {li}: an id differs where the oracle margin is {worst:.3e}'
    return y, y2, ref, differ, total


def guarded_input(sd, hyper, shape, seed, make, guard=5 * O.TAU, tries=40):
    """The first of ``make(shape, seed)``, ``make(shape, seed + 1)``, ... on which the float64 oracle, running free, takes every category
    decision with a relative top-two margin of at least ``guard`` (5 TAU by default).  On such an input a correct float32 implementation
    decides as the oracle does, so the 0.2 % cap on differing decisions holds with none to spare even where 0.2 % of the decisions is less
    than one.  The choice looks at the oracle alone."""
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    for s in range(seed, seed + tries):
        x = make(shape, s)
        rec = {}
        with torch.no_grad():
            O.atd_forward(sd64, x.double(), hyper, record=rec)
        if min(mg.min().item() for mg in rec['margin']) >= guard:
            return x
    raise AssertionError(f'no guarded ATD input of shape {shape} among {tries} seeds from {seed}')
