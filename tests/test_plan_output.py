"""The output / input contract of ``Plan`` on the host: hand-filled descriptors over CPU tensors, with the library's launchers replaced by
recorders of the pointers they would pass (no library, no GPU); and, on the GPU, one positional launch whose pointer arguments follow the
output and the input like descriptor fields."""

import weakref

import pytest
import torch

from resselt_amd.engine import lib as L
from resselt_amd.engine import ops
from resselt_amd.engine.base import Plan

N, CH, H, W = 2, 3, 8, 8


def _recording_plan(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, 'current_stream_ptr', lambda device: 0)
    monkeypatch.setattr(L, 'conv2d_list', lambda arr, stream: seen.append([(p.out_nchw, p.out_base) for p in arr]))
    monkeypatch.setattr(L, 'launch', lambda name, p, stream: seen.append((name, p.out_nchw, p.x_f32)))
    return Plan('cpu'), seen


def _conv(out: torch.Tensor, base: torch.Tensor | None = None) -> L.ConvParams:
    p = L.ConvParams()
    p.batch, p.H, p.W, p.ksize, p.cin_planes, p.cout, p.products = out.shape[0], H, W, 3, 1, CH, 1
    p.out_nchw, p.out_dtype = out.data_ptr(), L.F32
    if base is not None:
        p.out_base = base.data_ptr()
    return p


def test_plan_output_and_input_are_rebound_per_forward(monkeypatch):
    plan, seen = _recording_plan(monkeypatch)
    scratch = plan.f32map(N, 8, H, W)
    y0 = plan.output((N, CH, H, W), torch.float32, crop=(6, 7))
    x0 = plan.input_ref((N, CH, H, W), torch.float32)
    plan.conv(_conv(y0[0:1], x0))
    plan.conv(_conv(y0[1:2]))  # a slice at a non-zero byte offset
    dp = L.DySampleParams()
    dp.x_f32, dp.out_nchw, dp.out_dtype = scratch.data_ptr(), y0.data_ptr(), L.F32
    plan.launch('rsa_dysample', dp)
    plan.flush()
    y0_ptr = y0.data_ptr()  # (x0 stays referenced here: no input below can take its address, so a re-pointed field shows)
    image = CH * H * W * 4

    assert plan.buffer_bytes() == scratch.numel() * 4  # the output is not a plan buffer
    assert plan.n_launches() == 3

    def forward(x):
        plan.feed(x)
        assert plan.conv_arrays[0][0].out_base == x.data_ptr()  # re-pointed when fed, before any step runs
        seen.clear()
        plan.run()
        return plan.take_output()

    x1 = torch.randn(N, CH, H, W)
    y1 = forward(x1)
    assert y1.shape == (N, CH, 6, 7)
    assert y1.data_ptr() == y0_ptr  # the first forward writes the placeholder
    assert seen == [[(y0_ptr, x1.data_ptr()), (y0_ptr + image, None)], ('rsa_dysample', y0_ptr, scratch.data_ptr())]

    x2 = torch.randn(N, CH, H, W)
    x2_ptr, x2_ref = x2.data_ptr(), weakref.ref(x2)
    y1.fill_(1.0)
    y2 = forward(x2)
    assert y2.shape == (N, CH, 6, 7) and y2.data_ptr() != y1.data_ptr()  # a fresh output
    base = y2.data_ptr()
    assert seen == [[(base, x2_ptr), (base + image, None)], ('rsa_dysample', base, scratch.data_ptr())]
    assert bool((y1 == 1.0).all())  # the first result is left alone

    del x2
    assert x2_ref() is None  # take_output let go of the input

    # a replay of the steps after take_output (what bench.py does) gets a valid output pointer and the last input's
    seen.clear()
    plan.run()
    held = plan.current_output()
    assert held is not None and seen[0][0] == (held.data_ptr(), x2_ptr)
    plan.release()
    assert plan.current_output() is None


def test_plan_crops_u8_nhwc_rows_and_columns(monkeypatch):
    plan, _ = _recording_plan(monkeypatch)
    y = plan.output((1, 10, 12, 3), torch.uint8, crop=(9, 11))
    plan.feed(torch.zeros((1, 5, 6, 3), dtype=torch.uint8))
    plan.run()
    out = plan.take_output()
    assert out.shape == (1, 9, 11, 3) and out.data_ptr() == y.data_ptr()


@pytest.mark.gpu
def test_positional_launch_follows_the_output_and_the_input(device):
    """``rsa_scale_add`` (out += gamma[c] * res on f32 NCHW4c maps) of a 1x4x8x8 map, with ``out`` the plan's output and ``res`` the caller's
    input: its argument list is resolved once, when the step is built, and the two pointers are re-pointed per forward.  Small integers times
    powers of two: every value is exact in f32, whether or not the kernel fuses the multiply-add."""
    shape = (1, 1, 8, 8, 4)
    plan = Plan(device)
    gamma = torch.tensor([0.5, 2.0, -1.0, 4.0], device=device)
    y0 = plan.output(shape, torch.float32)
    x0 = plan.input_ref(shape, torch.float32)
    plan.call(lambda: plan.current_output().fill_(3.0))
    plan.launch('rsa_scale_add', dict(res=x0, gamma=gamma, out=y0, batch=1, H=8, W=8, C=4))
    plan.flush()
    y0_ptr = y0.data_ptr()
    assert plan.n_launches() == 1
    del y0

    def forward(x):
        plan.feed(x)
        plan.run()
        return plan.take_output()

    g = torch.Generator().manual_seed(3)
    x1, x2 = (torch.randint(-64, 64, shape, generator=g).float().to(device) for _ in range(2))
    y1 = forward(x1)
    y1_copy = y1.clone()
    y2 = forward(x2)
    torch.cuda.synchronize()
    assert y1.data_ptr() == y0_ptr and y2.data_ptr() != y1.data_ptr()  # the placeholder first, then a fresh tensor
    assert torch.equal(y2, 3.0 + x2 * gamma) and not torch.equal(y2, y1)
    assert torch.equal(y1, y1_copy) and torch.equal(y1, 3.0 + x1 * gamma)  # the first result is left alone
    L.check_status('positional launch')
