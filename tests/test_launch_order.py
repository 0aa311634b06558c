"""Serpentine order per launch (``rsa_conv2d_list_assign_tile_order``): the library walks a descriptor list the way
``rsa_conv2d_list`` launches it and alternates ``tile_order`` per LAUNCH, both halves of a fused pair carrying the pair's order.  Host logic
only: the descriptors are built by hand with fake non-null pointers and nothing is launched."""

import ctypes

import pytest

from resselt_amd.engine import lib as L
from resselt_amd.engine.base import Plan
from resselt_amd.engine.tensors import PF_F16

E_ARG = -1  # RSA_E_ARG
WL_PAIRS = 1  # RSA_WL_PAIRS (csrc/common.h)
BUF, OTHER, WEIGHTS = 0x10000, 0x90000, 0x200000  # fake 16-byte aligned addresses
H, W = 40, 70


def _growth(cin_planes: int, buf: int = BUF) -> L.ConvParams:
    """A growth convolution of a dense block in the one-product fp16 mode: reads ``cin_planes`` planes of ``buf`` and writes the four behind
    them (3x3, 32 couts, bias-free LeakyReLU into hi-only fp16 planes, pair weight layout)."""
    p = L.ConvParams()
    p.batch, p.H, p.W, p.ksize, p.cin_planes, p.cout, p.products = 1, H, W, 3, cin_planes, 32, 1
    p.in_fmt = p.out_fmt = p.res_fmt = PF_F16
    p.in_hi = p.out_hi = buf
    p.in_plane_stride = p.out_plane_stride = H * W
    p.in_batch_stride = p.out_batch_stride = 24 * H * W
    p.out_plane_off = cin_planes
    p.w_packed, p.w_layout = WEIGHTS, WL_PAIRS
    p.act, p.act_param = L.ACT_LRELU, 0.2
    return p


def _single() -> L.ConvParams:
    """A layer that fuses with neither neighbour: 64 output channels into another buffer."""
    p = _growth(24)
    p.cout, p.out_hi, p.out_plane_off = 64, OTHER, 0
    return p


def _block_list():
    """single, pair, pair, single, pair, pair, single: (descriptor array, first descriptor of every launch, whether it is fused)."""
    descs = [_single(), _growth(8), _growth(12), _growth(16), _growth(20), _single(), _growth(8), _growth(12), _growth(16), _growth(20), _single()]
    launches = [(0, False), (1, True), (3, True), (5, False), (6, True), (8, True), (10, False)]
    return (L.ConvParams * len(descs))(*descs), launches


def _orders(arr):
    return [p.tile_order for p in arr]


@pytest.fixture
def fusion_on():
    L.set_pair_fusion(1)
    try:
        yield
    finally:
        L.set_pair_fusion(-1)


def test_the_hand_built_list_has_the_shape_it_claims(fusion_on):
    arr, launches = _block_list()
    fusable = [L.conv_pair_fusable(arr[i], arr[i + 1]) for i in range(len(arr) - 1)]
    #          s-a    a-b   b-c    c-d   d-s    s-a    a-b   b-c    c-d   d-s
    assert fusable == [False, True, True, True, False, False, True, True, True, False]  # (b, c) is fusable too: the walk is greedy from the left
    assert [i for i, fused in launches if fused] == [1, 3, 6, 8]


@pytest.mark.parametrize('first', [0, 1])
def test_orders_alternate_per_launch_and_pair_halves_agree(fusion_on, first):
    arr, launches = _block_list()
    for p in arr:
        p.tile_order = 1 - first  # whatever stood there is overwritten
    assert L.conv_list_assign_tile_order(arr, first) == (first + len(launches)) & 1
    for k, (i, fused) in enumerate(launches):
        assert arr[i].tile_order == (first + k) & 1, (k, i)
        if fused:
            assert arr[i + 1].tile_order == arr[i].tile_order, (k, i)
    per_launch = [arr[i].tile_order for i, _ in launches]
    assert all(a != b for a, b in zip(per_launch, per_launch[1:]))


@pytest.mark.parametrize('first', [0, 1])
def test_next_order_of_an_empty_list_and_a_null_next_order(first):
    lib = L.load()
    empty = (L.ConvParams * 0)()
    assert L.conv_list_assign_tile_order(empty, first) == first
    one = (L.ConvParams * 1)(_single())
    nxt = ctypes.c_int32(7)
    assert lib.rsa_conv2d_list_assign_tile_order(one, 0, first, ctypes.byref(nxt)) == 0 and nxt.value == first and one[0].tile_order == 0  # n = 0: nothing written
    assert lib.rsa_conv2d_list_assign_tile_order(one, 1, first, None) == 0 and one[0].tile_order == first


def test_without_fusion_the_same_list_alternates_per_descriptor():
    arr, _ = _block_list()
    L.set_pair_fusion(0)
    try:
        assert L.conv_list_assign_tile_order(arr, 0) == len(arr) & 1
        assert _orders(arr) == [k & 1 for k in range(len(arr))]
        assert L.conv_list_assign_tile_order(arr, 1) == (1 + len(arr)) & 1
        assert _orders(arr) == [(1 + k) & 1 for k in range(len(arr))]
    finally:
        L.set_pair_fusion(-1)


def test_a_list_without_a_fusable_pair_keeps_per_descriptor_orders(fusion_on):
    arr = (L.ConvParams * 5)(*[_single() for _ in range(5)])
    assert L.conv_list_assign_tile_order(arr, 0) == 1
    assert _orders(arr) == [0, 1, 0, 1, 0]


def test_argument_errors():
    lib = L.load()
    arr, _ = _block_list()
    nxt = ctypes.c_int32(7)
    for args in ((None, 1, 0), (arr, -1, 0), (arr, len(arr), 2), (arr, len(arr), -1)):
        assert lib.rsa_conv2d_list_assign_tile_order(*args, ctypes.byref(nxt)) == E_ARG, args
        assert b'rsa_conv2d_list_assign_tile_order' in lib.rsa_last_error_string()
    assert nxt.value == 7 and _orders(arr) == [0] * len(arr)  # a refused call writes nothing


def test_plan_flush_assigns_per_launch_and_carries_the_parity_across_lists(fusion_on, monkeypatch):
    """``Plan.conv`` alternates per descriptor; ``Plan.flush`` hands the list to the library with the plan's running launch parity.  A plan
    without a fusable pair is unchanged field for field; ``RSA_SERPENTINE=desc`` (the glue call skipped) keeps the per-descriptor orders."""
    from resselt_amd.engine import base

    descs = [_single(), _growth(8), _growth(12), _growth(16), _growth(20), _single()]
    plan = Plan('cpu')
    for p in descs:
        plan.conv(p)
    first = plan.flush()
    assert _orders(first) == [0, 1, 1, 0, 0, 1]  # four launches
    for p in descs:
        plan.conv(p)
    second = plan.flush()
    assert _orders(second) == [0, 1, 1, 0, 0, 1]  # launch parity 0 again after four launches (the descriptor parity is 0 too: six layers)
    plan.conv(_single())
    assert _orders(plan.flush()) == [0]
    L.set_pair_fusion(0)
    plan.reassign_launch_orders()
    assert _orders(first) + _orders(second) == [k & 1 for k in range(12)] and _orders(plan.conv_arrays[2]) == [0]
    L.set_pair_fusion(1)
    plan.reassign_launch_orders()
    assert _orders(first) == _orders(second) == [0, 1, 1, 0, 0, 1] and _orders(plan.conv_arrays[2]) == [0]

    plain = Plan('cpu')
    for _ in range(3):
        plain.conv(_single())
    a = plain.flush()
    for _ in range(2):
        plain.conv(_single())
    assert _orders(a) + _orders(plain.flush()) == [0, 1, 0, 1, 0]

    monkeypatch.setattr(base, '_SERPENTINE_PER_LAUNCH', False)
    desc = Plan('cpu')
    for p in descs:
        desc.conv(p)
    assert _orders(desc.flush()) == [0, 1, 0, 1, 0, 1]
