"""C-ABI facts of the PLKSR additions that need no GPU: existing convolution descriptors keep dispatching to the kernels they used
before (the EA gate is a separate streaming kernel, not a new epilogue), and the new entry points check their arguments."""

import ctypes as C

import pytest

from resselt_amd.engine import lib as L


def _desc(ksize, cin_planes, cout, products, act=0, fmt=0, out='planes', res=False, H=64, W=64):
    p = L.ConvParams()
    p.batch, p.H, p.W, p.ksize, p.cin_planes, p.cout, p.products = 1, H, W, ksize, cin_planes, cout, products
    p.in_fmt = p.out_fmt = p.res_fmt = fmt
    p.act = act
    p.in_hi, p.in_lo = 16, (16 if products == 3 else None)
    p.in_plane_stride = p.in_batch_stride = H * W
    if out == 'planes':
        p.out_hi, p.out_lo = 16, (16 if products == 3 else None)
        p.out_plane_stride, p.out_batch_stride = H * W, H * W * ((cout + 7) // 8)
    elif out == 'f32':
        p.out_f32 = 16
    else:
        p.out_nchw, p.pixel_shuffle = 16, 4
    if res:
        p.res1 = 16
    p.w_layout = L.load().rsa_conv_weight_layout(C.byref(p))
    return p


@pytest.mark.parametrize('args, name', [
    (dict(ksize=3, cin_planes=8, cout=32, products=1, act=L.ACT_LRELU, fmt=1), 'rsa::conv_ring<2,0,0,0,f16,1> (Cout<=32, one fp16 product)'),  # RRDBNet growth conv
    (dict(ksize=3, cin_planes=8, cout=64, products=3, act=L.ACT_LRELU), 'rsa::conv_ring<1,UP,0> (Cout 49..64)'),  # RRDBNet trunk, three products
    (dict(ksize=3, cin_planes=6, cout=48, products=1, act=L.ACT_SILU, fmt=1),
     'rsa::conv_ring<3,0,0,HM,f16,1,XRES 3> (SPAN-family 48-channel layer, one fp16 product, weights resident in LDS, direct epilogue)'),  # SPAN
    (dict(ksize=3, cin_planes=8, cout=64, products=1, act=L.ACT_PRELU, fmt=1), 'rsa::conv_ring<1,0,0,0,f16,1> (Cout 49..64, one fp16 product)'),  # Compact
    (dict(ksize=3, cin_planes=8, cout=48, products=3, out='nchw'), 'rsa::conv_ring<3,0,1,HM> (Cout 33..48, final store)'),  # final store
    (dict(ksize=1, cin_planes=24, cout=48, products=3, out='f32', res=True), 'rsa::conv_kernel'),  # k1 with an f32 residual
])  # fmt: skip
def test_existing_descriptors_keep_their_kernel(args, name):
    assert L.load().rsa_conv_kernel_name(C.byref(_desc(**args))).decode() == name


def test_version_unchanged():
    assert L.load().rsa_version() == 400


def test_plk_weight_bytes():
    lib = L.load()
    assert lib.rsa_plk_packed_weight_bytes(17, 2, 3) == 2 * 73 * 1 * 2 * 64 * 16
    assert lib.rsa_plk_packed_weight_bytes(17, 3, 1) == 3 * 73 * 2 * 1 * 64 * 16
    assert lib.rsa_plk_packed_weight_bytes(16, 2, 3) < 0 and lib.rsa_plk_packed_weight_bytes(33, 2, 3) < 0
    assert lib.rsa_plk_packed_weight_bytes(17, 9, 3) < 0


def test_new_entry_points_reject_bad_arguments():
    lib = L.load()
    p = L.PlkConvParams()
    p.batch, p.H, p.W, p.ksize, p.planes, p.products = 1, 8, 8, 16, 2, 3
    assert lib.rsa_plk_conv(C.byref(p), None) == -2  # even kernel
    p.ksize, p.planes = 17, 9
    assert lib.rsa_plk_conv(C.byref(p), None) == -2  # pdim > 64
    p.planes = 2
    assert lib.rsa_plk_conv(C.byref(p), None) == -1  # null operands
    assert lib.rsa_group_norm_stats(None, 1, 8, 8, 32, 4, 1e-5, None, None, None) == -1
    assert lib.rsa_group_norm_workspace_bytes(1, 8, 8, 4) == 4 * 4 * 4  # one chunk, four groups, four floats each
    assert lib.rsa_ea_gate(C.byref(L.EaGateParams()), None) == -1
    assert lib.rsa_group_norm_apply(C.byref(L.GroupNormApplyParams()), None) == -1
