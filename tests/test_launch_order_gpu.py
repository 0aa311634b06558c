"""Serpentine order per launch on a real RRDBNet plan: the sweep direction alternates between consecutive LAUNCHES of the
trunk -- a fused pair of growth convolutions is one of them -- and the result does not depend on the directions at all.

RRDBNet with two blocks on a 1 x 3 x 40 x 70 input: 3 x 3 tiles for the pair kernel (16 x 30) and for conv5 (16 x 32), ragged on both axes; a
smaller map has one tile row, where both directions are the same walk."""

import pytest
import torch

import resselt_amd
from resselt_amd.engine import base
from resselt_amd.engine import lib as L
from resselt_amd.utils import synth

pytestmark = pytest.mark.gpu

NB = 2
TRUNK = 1 + 15 * NB  # descriptor index of the trunk convolution: conv_first, then five layers in each of three dense blocks per RRDB


@pytest.fixture(scope='module')
def frame():
    return synth.rrdbnet_state_dict(nb=NB, seed=21), synth.synth_input((1, 3, 40, 70), seed=21)


def _model(sd, device):
    m = resselt_amd.load_from_state_dict(dict(sd)).to(device)
    assert m.precision == 'auto' and m.resolved_precision() == 'mixed'
    return m


def _descriptors(m):
    return [p for arr in m.last_plan().conv_arrays for p in arr]


def _launches(descs):
    """(first descriptor, fused) of every launch ``rsa_conv2d_list`` makes of ``descs``."""
    out, i = [], 0
    while i < len(descs):
        fused = i + 1 < len(descs) and L.conv_pair_fusable(descs[i], descs[i + 1])
        out.append((i, fused))
        i += 2 if fused else 1
    return out


def test_rrdbnet_launch_directions_alternate_and_results_do_not_move(device, frame, monkeypatch):
    sd, x = frame
    x = x.to(device)
    m = _model(sd, device)
    y = m(x)
    torch.cuda.synchronize()

    # (a) strict alternation per launch from conv_first to the trunk convolution; the halves of a fused pair agree
    assert len(m.last_plan().conv_arrays) == 1  # one band: the whole forward is one list
    descs = _descriptors(m)
    launches = [(i, fused) for i, fused in _launches(descs) if i <= TRUNK]
    assert launches[0] == (0, False) and launches[-1] == (TRUNK, False)
    assert len(launches) == 2 + 9 * NB and sum(fused for _, fused in launches) == 6 * NB  # per dense block: pair, pair, conv5
    for k, (i, fused) in enumerate(launches):
        assert descs[i].tile_order == k & 1, (k, i)
        if fused:
            assert descs[i + 1].tile_order == descs[i].tile_order, (k, i)
    assert all(descs[i].H > 32 and descs[i].W > 64 for i, _ in launches)  # three tile rows and columns

    # (b) bit-identical to the same model without the serpentine order, and to the per-descriptor order (the glue call skipped)
    flat = _model(sd, device)
    build = flat._build_plan

    def build_without_serpentine(plan, *args, **kwargs):
        plan.serpentine = False
        return build(plan, *args, **kwargs)

    flat._build_plan = build_without_serpentine
    y_flat = flat(x)
    assert {p.tile_order for p in _descriptors(flat)} == {0}

    monkeypatch.setattr(base, '_SERPENTINE_PER_LAUNCH', False)
    per_desc = _model(sd, device)
    y_desc = per_desc(x)
    assert [p.tile_order for p in _descriptors(per_desc)] == [k & 1 for k in range(len(descs))]
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert torch.equal(y, y_flat)
    assert torch.equal(y, y_desc)

    # (c) no hand-off of the ring schedule ran into its spin bound
    assert L.ring_aborts() == 0
    L.check_status('launch order')
