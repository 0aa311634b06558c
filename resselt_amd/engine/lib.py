"""ctypes binding of ``libresselt_amd.so`` (C-ABI declared in ``include/resselt_amd.h``).

The library is the product: there is no CPU or PyTorch fallback behind these wrappers.
``load()`` raises ``RuntimeError`` when the shared object is missing or a symbol is absent,
and every call raises ``RuntimeError`` with ``rsa_last_error_string()`` on a non-zero status.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_LIB_NAME = 'libresselt_amd.so'
_lib: Optional[C.CDLL] = None

# enum rsa_act
ACT_NONE, ACT_LRELU, ACT_MISH, ACT_SILU, ACT_GELU, ACT_SPAB_GATE, ACT_PRELU = range(7)
# enum rsa_dtype
F32, F16, BF16, U8 = range(4)
LO8_RES1, LO8_RES2, LO8_OUT = 1, 2, 4  # rsa_conv_params.lo8_flags
# enum rsa_plane_fmt
PF_BF16, PF_F16 = range(2)
E_INTERNAL = -4
E_UNSUPPORTED = -2
E_FP16_RANGE = -5  # RSA_E_FP16_RANGE


def _i32(*names: str) -> list:
    return [(k, C.c_int32) for k in names]


def _i64(*names: str) -> list:
    return [(k, C.c_int64) for k in names]


def _f32(*names: str) -> list:
    return [(k, C.c_float) for k in names]


def _ptr(*names: str) -> list:
    return [(k, C.c_void_p) for k in names]


def _plane_fields(prefix: str) -> list:
    """A split-plane operand: what ``Planes.bind(params, prefix)`` fills."""
    return _ptr(f'{prefix}_hi', f'{prefix}_lo') + _i64(f'{prefix}_plane_stride', f'{prefix}_batch_stride')


# Mirrors of the descriptors in include/resselt_amd.h: field order and types are the ABI (tests/test_capi_headers.py compares every one of
# them with the header).
class ConvParams(C.Structure):
    """Mirror of ``struct rsa_conv_params`` (include/resselt_amd.h); field order is the ABI."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'ksize', 'upsample2x', 'cin_planes', 'cout', 'products') + _plane_fields('in') + _ptr('w_packed', 'bias')
        + _i32('act') + _f32('act_param', 'alpha') + _ptr('res1') + _f32('beta') + _ptr('res2', 'out_hi', 'out_lo') + _i32('out_plane_off')
        + _i64('out_plane_stride', 'out_batch_stride') + _ptr('out_f32', 'out_nchw') + _i32('out_dtype', 'pixel_shuffle')
        + _f32('out_scale') + _ptr('out_shift', 'act_vec', 'out_base') + _i32('out_base_div', 'out_base_h', 'out_base_w', 'w_layout')
        + _ptr('res1_hi', 'res1_lo', 'res2_hi', 'res2_lo') + _i64('res_plane_stride', 'res_batch_stride')
        + _i32('in_fmt', 'out_fmt', 'res_fmt', 'tile_order', 'lo8_flags', 'reserved_lo8') + _i64('lo8_batch_stride') + _ptr('pool_sums')
    )


class DySampleParams(C.Structure):
    """Mirror of ``struct rsa_dysample_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'groups', 'scale', 'out_ch') + _ptr('x_f32', 'offscope', 'init_pos', 'end_w', 'end_b', 'out_nchw')
        + _i32('out_dtype')
    )


class LayerNormParams(C.Structure):
    """Mirror of ``struct rsa_layernorm_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C') + _f32('eps') + _ptr('x_f32', 'gamma', 'beta') + _plane_fields('out') + _ptr('out_f32')
        + _i32('out_fmt', 'reserved0')
    )


class SwinAttnBlockParams(C.Structure):
    """Mirror of ``struct rsa_swin_attn_block_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'heads', 'window', 'shift', 'products') + _f32('eps')
        + _ptr('x', 'gamma', 'beta', 'wqkv', 'bqkv', 'bias_frag16', 'wproj', 'bproj', 'out')
    )


class SwinMlpBlockParams(C.Structure):
    """Mirror of ``struct rsa_swin_mlp_block_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'hidden', 'products') + _f32('eps') + _ptr('x', 'gamma', 'beta', 'w1', 'b1', 'w2', 'b2', 'out')
        + _plane_fields('out') + _i32('fmt', 'reserved0')
    )


class SwinBlockParams(C.Structure):
    """Mirror of ``struct rsa_swin_block_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'heads', 'window', 'shift', 'hidden', 'products') + _f32('eps')
        + _ptr('x', 'gamma1', 'beta1', 'wqkv', 'bqkv', 'bias_frag16', 'wproj', 'bproj', 'gamma2', 'beta2', 'w1', 'b1', 'w2', 'b2')
        + _ptr('out') + _plane_fields('out') + _i32('fmt', 'reserved0')
    )


class WindowAttnParams(C.Structure):
    """Mirror of ``struct rsa_window_attn_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'heads', 'window', 'shift', 'products') + _plane_fields('qkv') + _ptr('bias_frag') + _plane_fields('out')


class RectAttnParams(C.Structure):
    """Mirror of ``struct rsa_rect_attn_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'Hp', 'Wp', 'win_h', 'win_w', 'shift_h', 'shift_w', 'heads', 'head0', 'heads_total', 'products')
        + _plane_fields('qkv') + _ptr('bias_frag') + _plane_fields('out')
        + _i32('kwin_h', 'kwin_w', 'kpad_h', 'kpad_w', 'head_chunks', 'fmt', 'reserved0')
    )


class ChannelAttnParams(C.Structure):
    """Mirror of ``struct rsa_channel_attn_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'heads', 'head_dim', 'products') + _ptr('q_hi', 'q_lo', 'k_hi', 'k_lo')
        + _i64('plane_stride', 'batch_stride') + _ptr('temperature', 'workspace', 'w_packed') + _i32('fmt', 'reserved1')
    )


class DwConvParams(C.Structure):
    """Mirror of ``struct rsa_dwconv_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'planes', 'act') + _plane_fields('in') + _ptr('weight', 'bias', 'stats', 'gamma', 'beta')
        + _plane_fields('mul') + _plane_fields('out') + _i32('fmt', 'reserved1')
    )


class ChannelGateParams(C.Structure):
    """Mirror of ``struct rsa_channel_gate_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'planes', 'hidden') + _plane_fields('in') + _ptr('w1', 'b1', 'w2', 'b2', 'workspace', 'gate')
        + _i32('relu', 'fmt')
    )


class GatedShuffleParams(C.Structure):
    """Mirror of ``struct rsa_gated_shuffle_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'g_planes', 'i_planes') + _plane_fields('f') + _plane_fields('c') + _ptr('gate') + _i64('gate_stride')
        + _plane_fields('out')
    )


class AimParams(C.Structure):
    """Mirror of ``struct rsa_aim_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'planes', 'hidden', 'mode') + _plane_fields('att') + _plane_fields('conv')
        + _ptr('gate', 'w1', 'b1', 'w2') + _f32('b2') + _plane_fields('out') + _i32('fmt', 'reserved1')
    )


class PlkConvParams(C.Structure):
    """Mirror of ``struct rsa_plk_conv_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'ksize', 'planes', 'products') + _plane_fields('in') + _ptr('w_packed', 'bias') + _plane_fields('out')
        + _i32('out_plane_off', 'fmt', 'reserved0', 'reserved1')
    )


class GroupNormApplyParams(C.Structure):
    """Mirror of ``struct rsa_group_norm_apply_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'groups', 'out_fmt') + _ptr('x_f32', 'stats', 'gamma', 'beta', 'skip_f32') + _plane_fields('out')
        + _ptr('out_f32') + _i32('reserved0', 'reserved1')
    )


class EaGateParams(C.Structure):
    """Mirror of ``struct rsa_ea_gate_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'C') + _ptr('g_f32') + _plane_fields('x') + _plane_fields('out') + _i32('fmt', 'reserved0')


class ResampleConvParams(C.Structure):
    """Mirror of ``struct rsa_resample_conv_params`` (rsa_deconv / rsa_conv_s2)."""

    _fields_ = (
        _i32('batch', 'ksize', 'stride', 'pad', 'cin_planes', 'cout', 'products', 'fmt') + _plane_fields('in')
        + _i32('in_W', 'in_y0', 'in_x0', 'in_h', 'in_w', 'act') + _f32('act_param') + _i32('reserved0') + _ptr('w_packed', 'bias')
        + _plane_fields('res') + _i32('res_W', 'res_y0', 'res_x0', 'out_H', 'out_W', 'out_y0', 'out_x0') + _plane_fields('out')
        + _ptr('out_f32') + _i32('reserved1')
    )


class RegionSEParams(C.Structure):
    """Mirror of ``struct rsa_region_se_params``."""

    _fields_ = (
        _i32('batch', 'planes', 'hidden', 'fmt') + _plane_fields('x') + _i32('W', 'y0', 'x0', 'h', 'w', 'reserved0')
        + _ptr('w1', 'b1', 'w2', 'b2', 'workspace', 'gate')
    )


class CuganInputParams(C.Structure):
    """Mirror of ``struct rsa_cugan_input_params``."""

    _fields_ = (
        _ptr('x') + _i32('dtype', 'batch', 'C', 'h', 'w', 'pad_top', 'pad_left', 'unshuffle') + _f32('in_scale', 'in_shift')
        + _i32('out_H', 'out_W', 'fmt') + _plane_fields('out') + _i32('reserved0')
    )


class CuganOutputParams(C.Structure):
    """Mirror of ``struct rsa_cugan_output_params``."""

    _fields_ = (
        _ptr('map') + _i32('batch', 'C', 'map_H', 'map_W', 'y0', 'x0', 'pixel_shuffle', 'out_h', 'out_w', 'dtype') + _ptr('out', 'base')
        + _i32('base_h', 'base_w', 'base_div') + _f32('base_scale', 'base_shift', 'out_shift', 'out_div') + _i32('reserved0')
    )


class GatedDwConvSegment(C.Structure):
    """Mirror of ``struct rsa_gated_dwconv_segment``."""

    _fields_ = _i32('planes', 'kh', 'kw', 'reserved0') + _ptr('weight', 'bias')


class GatedDwConvParams(C.Structure):
    """Mirror of ``struct rsa_gated_dwconv_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'fmt', 'i_planes', 'n_segments') + [('seg', GatedDwConvSegment * 4)] + _plane_fields('g')
        + _plane_fields('x') + _plane_fields('out')
    )


class BilinearAddParams(C.Structure):
    """Mirror of ``struct rsa_bilinear_add_params``."""

    _fields_ = _i32('batch', 'C', 'h', 'w', 'pad_h', 'pad_w', 'scale', 'dtype', 'out_H', 'out_W', 'out_h', 'out_w') + _ptr('x', 'out')


class RgAttnParams(C.Structure):
    """Mirror of ``struct rsa_rg_attn_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'heads', 'nkeys', 'dim_qk', 'dim_v', 'products', 'fmt', 'reserved0') + _plane_fields('q')
        + _plane_fields('k') + _plane_fields('v') + _plane_fields('out')
    )


class RgReduceParams(C.Structure):
    """Mirror of ``struct rsa_rg_reduce_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'planes', 'times', 'fmt') + _plane_fields('in') + _ptr('weight', 'bias') + _plane_fields('out')


class FdatInteractParams(C.Structure):
    """Mirror of ``struct rsa_fdat_interact_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'mode', 'fmt') + _plane_fields('a') + _plane_fields('c')
        + _ptr('cm', 'w', 'x', 'x_out', 'gamma', 'beta') + _f32('eps') + _i32('reserved0') + _plane_fields('out')
    )


class LdaOffsetsParams(C.Structure):
    """Mirror of ``struct rsa_lda_offsets_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'Hout', 'Wout', 'hidden', 'groups', 'fmt') + _plane_fields('q') + _ptr('dw_weight', 'gamma', 'beta')
        + _f32('eps') + _i32('reserved0') + _plane_fields('out')
    )


class LdaAttnParams(C.Structure):
    """Mirror of ``struct rsa_lda_attn_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'Hout', 'Wout', 'hidden', 'C', 'groups', 'fmt') + _f32('range', 'scale') + _i32('reserved0')
        + _plane_fields('q') + _plane_fields('k') + _plane_fields('v') + _ptr('offset', 'rpb') + _plane_fields('out')
    )


class OmniAttnParams(C.Structure):
    """Mirror of ``struct rsa_omni_attn_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'ws', 'heads', 'head_dim', 'grid', 'fmt') + _plane_fields('qkv')
        + _ptr('bias_table', 'temperature', 'workspace') + _plane_fields('out')
    )


class GeluGateDwConvParams(C.Structure):
    """Mirror of ``struct rsa_gelu_gate_dwconv_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'planes', 'fmt', 'reserved0') + _plane_fields('in') + _ptr('weight') + _plane_fields('out')


class EsaConvParams(C.Structure):
    """Mirror of ``struct rsa_esa_conv_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'Hout', 'Wout', 'cin', 'cout', 'stride', 'pad', 'reserved0') + _ptr('in_', 'weight', 'bias', 'out')


class EsaApplyParams(C.Structure):
    """Mirror of ``struct rsa_esa_apply_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'C', 'f', 'Hc', 'Wc', 'fmt') + _ptr('x', 'c1', 'c3', 'wf', 'bf', 'w4', 'b4', 'out') + _plane_fields('out')


class AtdDictParams(C.Structure):
    """Mirror of ``struct rsa_atd_dict_params``."""

    _fields_ = _i32('batch', 'C', 'm', 'rc') + _ptr('td', 'wk', 'bk', 'wv', 'bv', 'kn', 'vt_hi', 'vt_lo')


class AtdCaParams(C.Structure):
    """Mirror of ``struct rsa_atd_ca_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'C', 'm', 'rc', 'products', 'reserved0')
        + _ptr('xn', 'wq', 'bq', 'kn', 'scale', 'vt_hi', 'vt_lo', 'sim', 'ids', 'out')
    )


class AtdAttnParams(C.Structure):
    """Mirror of ``struct rsa_atd_attn_params``."""

    _fields_ = (
        _i32('batch', 'H', 'W', 'heads', 'head_dim', 'mode', 'ws', 'shift', 'gs', 'products') + _f32('scale') + _i32('reserved0')
        + _plane_fields('qkv') + _ptr('bias_table', 'perm') + _plane_fields('out')
    )


class AtdDwConvParams(C.Structure):
    """Mirror of ``struct rsa_atd_dwconv_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'planes') + _plane_fields('in') + _ptr('weight', 'bias') + _plane_fields('out')


class AtdRefineParams(C.Structure):
    """Mirror of ``struct rsa_atd_refine_params``."""

    _fields_ = _i32('batch', 'H', 'W', 'C', 'm') + _f32('eps') + _ptr('sim', 'x', 'gamma', 'beta', 'sigma', 'td', 'workspace')


def _conv(*names: str) -> list:
    return [(k, C.POINTER(ConvParams)) for k in names]


def _descriptor(struct) -> tuple:
    """An entry point that takes ``(const struct* p, void* stream)`` and returns a status."""
    return (C.c_int, [('p', C.POINTER(struct))] + _ptr('stream'))


# Every entry point include/resselt_amd.h declares: name -> (restype, [(parameter name, ctype), ...]), the header's names in the header's
# order, the trailing ``void* stream`` included.  ``load()`` sets argtypes / restype from it, ``bind`` resolves keyword arguments against
# it, and tests/test_capi_headers.py compares every row with its prototype.  A new entry point = its prototype there + its row here.
SIGNATURES = {
    'rsa_conv2d': _descriptor(ConvParams),
    'rsa_conv2d_list': (C.c_int, _conv('list') + _i32('n') + _ptr('stream')),
    'rsa_conv2d_pair': (C.c_int, _conv('a', 'b') + _ptr('stream')),
    'rsa_conv_pair_fusable': (C.c_int, _conv('a', 'b')),
    'rsa_check_status': (C.c_int, []),
    'rsa_check_finite': (C.c_int, _ptr('data') + _i32('dtype') + _i64('count') + _ptr('stream')),
    'rsa_packed_weight_bytes': (C.c_int64, _i32('cout', 'cin_planes', 'ksize', 'products')),
    'rsa_packed_weight_bytes_layout': (C.c_int64, _i32('cout', 'cin_planes', 'ksize', 'products', 'layout')),
    'rsa_conv_cout_tiles': (C.c_int, _i32('cout')),
    'rsa_conv_pool_slots': (C.c_int, _conv('p')),
    'rsa_conv_weight_layout': (C.c_int, _conv('p')),
    'rsa_pack_weights': (C.c_int, _ptr('w_oihw') + _i32('cout', 'cin', 'cin_planes', 'ksize', 'products', 'layout', 'fmt') + _ptr('out', 'stream')),
    'rsa_conv_kernel_name': (C.c_char_p, _conv('p')),
    'rsa_debug_ring_aborts': (C.c_int, []),
    'rsa_debug_set_ring_spin_limit': (C.c_int, _i32('polls')),
    'rsa_debug_set_ring': (C.c_int, _i32('mode')),
    'rsa_debug_set_pair': (C.c_int, _i32('mode')),
    'rsa_nchw_to_planes': (C.c_int, _ptr('x') + _i32('dtype', 'batch', 'C', 'H', 'W', 'src_h', 'src_w', 'unshuffle') + _ptr('mean') + _f32('scale') + _plane_fields('out') + _i32('out_fmt') + _ptr('stream')),
    'rsa_planes_to_nchw': (C.c_int, _ptr('hi', 'lo') + _i64('plane_stride', 'batch_stride') + _i32('batch', 'C', 'H', 'W', 'fmt') + _ptr('out', 'stream')),
    'rsa_dysample': _descriptor(DySampleParams),
    'rsa_layernorm': _descriptor(LayerNormParams),
    'rsa_window_attention': _descriptor(WindowAttnParams),
    'rsa_swin_attn_block': _descriptor(SwinAttnBlockParams),
    'rsa_swin_mlp_block': _descriptor(SwinMlpBlockParams),
    'rsa_swin_block': _descriptor(SwinBlockParams),
    'rsa_rect_attention': _descriptor(RectAttnParams),
    'rsa_channel_attn_workspace_bytes': (C.c_int64, _i32('batch', 'H', 'W', 'heads')),
    'rsa_channel_attention_weights': _descriptor(ChannelAttnParams),
    'rsa_dwconv3x3': _descriptor(DwConvParams),
    'rsa_dwconv5x5': _descriptor(DwConvParams),
    'rsa_plane_stats': (C.c_int, _ptr('in_hi', 'in_lo') + _i64('plane_stride', 'batch_stride') + _i32('batch', 'H', 'W', 'C') + _f32('eps') + _ptr('stats', 'stream')),
    'rsa_plane_stats_fmt': (C.c_int, _ptr('in_hi', 'in_lo') + _i64('plane_stride', 'batch_stride') + _i32('batch', 'H', 'W', 'C') + _f32('eps') + _i32('fmt') + _ptr('stats', 'stream')),
    'rsa_channel_gate_workspace_bytes': (C.c_int64, _i32('batch', 'H', 'W', 'planes')),
    'rsa_channel_gate': _descriptor(ChannelGateParams),
    'rsa_aim_combine': _descriptor(AimParams),
    'rsa_gated_add': (C.c_int, _ptr('x_hi', 'x_lo') + _i64('plane_stride', 'batch_stride') + _i32('batch', 'H', 'W', 'C') + _ptr('gate') + _f32('scale') + _ptr('base_f32', 'out_f32', 'stream')),
    'rsa_rmsnorm': (C.c_int, _ptr('x_f32') + _i32('batch', 'H', 'W', 'C') + _f32('eps') + _ptr('scale', 'offset') + _plane_fields('out') + _ptr('stream')),
    'rsa_unshuffle_pool': (C.c_int, _plane_fields('in') + _i32('batch', 'H', 'W', 'planes') + _ptr('unshuffled_f32') + _plane_fields('pool') + _ptr('stream')),
    'rsa_gated_shuffle_mul': _descriptor(GatedShuffleParams),
    'rsa_plk_packed_weight_bytes': (C.c_int64, _i32('ksize', 'planes', 'products')),
    'rsa_plk_conv': _descriptor(PlkConvParams),
    'rsa_group_norm_workspace_bytes': (C.c_int64, _i32('batch', 'H', 'W', 'groups')),
    'rsa_group_norm_stats': (C.c_int, _ptr('x_f32') + _i32('batch', 'H', 'W', 'C', 'groups') + _f32('eps') + _ptr('workspace', 'stats', 'stream')),
    'rsa_group_norm_apply': _descriptor(GroupNormApplyParams),
    'rsa_ea_gate': _descriptor(EaGateParams),
    'rsa_resample_packed_weight_bytes': (C.c_int64, _i32('ksize', 'stride', 'transposed', 'cin_planes', 'cout', 'products')),
    'rsa_deconv': _descriptor(ResampleConvParams),
    'rsa_conv_s2': _descriptor(ResampleConvParams),
    'rsa_region_se_workspace_bytes': (C.c_int64, _i32('batch', 'h', 'planes')),
    'rsa_region_se': _descriptor(RegionSEParams),
    'rsa_cugan_input': _descriptor(CuganInputParams),
    'rsa_cugan_output': _descriptor(CuganOutputParams),
    'rsa_gated_dwconv': _descriptor(GatedDwConvParams),
    'rsa_bilinear_add': _descriptor(BilinearAddParams),
    'rsa_rg_attention': _descriptor(RgAttnParams),
    'rsa_rg_reduce': _descriptor(RgReduceParams),
    'rsa_layernorm_gelu': _descriptor(LayerNormParams),
    'rsa_scale_add': (C.c_int, _ptr('res', 'gamma', 'out') + _i32('batch', 'H', 'W', 'C') + _ptr('stream')),
    'rsa_fdat_interact': _descriptor(FdatInteractParams),
    'rsa_pa_gate': (C.c_int, _ptr('x_hi', 'x_lo', 'logit_hi', 'logit_lo') + _i64('plane_stride', 'batch_stride') + _i32('batch', 'H', 'W', 'planes') + _f32('slope') + _i32('fmt') + _ptr('out_hi', 'out_lo', 'stream')),
    'rsa_lda_offsets': _descriptor(LdaOffsetsParams),
    'rsa_lda_attention': _descriptor(LdaAttnParams),
    'rsa_omni_window_attention': _descriptor(OmniAttnParams),
    'rsa_omni_channel_attn_workspace_bytes': (C.c_int64, _i32('batch', 'H', 'W', 'ws', 'heads', 'head_dim', 'grid')),
    'rsa_omni_channel_attention': _descriptor(OmniAttnParams),
    'rsa_gelu_gate_dwconv': _descriptor(GeluGateDwConvParams),
    'rsa_omni_gate_scale': (C.c_int, _ptr('in_hi', 'in_lo') + _i64('plane_stride', 'batch_stride') + _i32('batch', 'H', 'W', 'planes') + _ptr('gate') + _i32('fmt') + _ptr('out_hi', 'out_lo', 'stream')),
    'rsa_esa_conv3x3': _descriptor(EsaConvParams),
    'rsa_esa_maxpool': (C.c_int, _ptr('in') + _i32('batch', 'C', 'H', 'W') + _ptr('out', 'stream')),
    'rsa_esa_apply': _descriptor(EsaApplyParams),
    'rsa_atd_dict': _descriptor(AtdDictParams),
    'rsa_atd_ca': _descriptor(AtdCaParams),
    'rsa_atd_sort_workspace_bytes': (C.c_int64, _i32('batch') + _i64('n')),
    'rsa_atd_sort': (C.c_int, _ptr('ids') + _i32('batch') + _i64('n') + _i32('m') + _ptr('perm', 'inv', 'workspace', 'stream')),
    'rsa_atd_attention': _descriptor(AtdAttnParams),
    'rsa_atd_dwconv': _descriptor(AtdDwConvParams),
    'rsa_atd_refine_workspace_bytes': (C.c_int64, _i32('batch', 'H', 'W', 'C', 'm')),
    'rsa_atd_refine': _descriptor(AtdRefineParams),
    'rsa_rcab_tail': (C.c_int, _ptr('pool_sums') + _i32('slots') + _ptr('w1', 'b1', 'w2', 'b2') + _i32('hidden') + _ptr('gate') + _plane_fields('y') + _plane_fields('x') + _plane_fields('out') + _i32('batch', 'H', 'W', 'C', 'fmt') + _ptr('stream')),
    'rsa_rcan_input': (C.c_int, _ptr('x') + _i32('dtype', 'batch', 'C', 'H', 'W') + _f32('scale') + _ptr('weight', 'bias', 'out', 'stream')),
    'rsa_image_u8_to_nchw': (C.c_int, _ptr('img') + _i32('batch', 'H', 'W', 'C') + _ptr('out') + _i32('dtype') + _ptr('stream')),
    'rsa_nchw_to_image_u8': (C.c_int, _ptr('x') + _i32('dtype', 'batch', 'C', 'H', 'W') + _ptr('img', 'stream')),
    'rsa_rmsnorm_torch': (C.c_int, _ptr('x_f32') + _i32('batch', 'H', 'W', 'C') + _f32('eps') + _ptr('weight') + _plane_fields('out') + _i32('fmt') + _ptr('stream')),
    'rsa_pixel_unshuffle2': (C.c_int, _ptr('x_f32') + _i32('batch', 'H', 'W', 'C') + _ptr('out_f32', 'stream')),
    'rsa_f32map_concat': (C.c_int, _ptr('a_nchw') + _i32('Ca') + _ptr('b_map') + _i32('Cb', 'batch', 'H', 'W') + _ptr('out_map', 'stream')),
    'rsa_fla_workspace_bytes': (C.c_int64, _i32('batch', 'tokens', 'head_dim')),
    'rsa_fla_reduce': (C.c_int, _plane_fields('qkv') + _i32('batch', 'H', 'W', 'head_dim', 'fmt') + _ptr('scale', 'factor', 'workspace') + _i64('workspace_bytes') + _ptr('stream')),
    'rsa_fla_apply': (C.c_int, _plane_fields('qkv') + _i32('batch', 'H', 'W', 'head_dim', 'fmt') + _ptr('scale', 'factor', 'workspace') + _i64('workspace_bytes') + _ptr('dwc_weight', 'dwc_bias') + _plane_fields('out') + _ptr('stream')),
    'rsa_eimn_query_chain': (C.c_int, _plane_fields('q') + _plane_fields('out') + _i32('batch', 'H', 'W', 'planes_a', 'planes_b', 'planes_c', 'gelu_in', 'fmt') + _ptr('w1', 'b1', 'w2', 'b2', 'stream')),
    'rsa_eimn_sal': (C.c_int, _plane_fields('in') + _plane_fields('out') + _i32('batch', 'H', 'W', 'planes', 'fmt') + _ptr('weight', 'bias', 'stream')),
    'rsa_eimn_silu_mul': (C.c_int, _plane_fields('f') + _plane_fields('v') + _plane_fields('out') + _i32('batch', 'H', 'W', 'planes', 'fmt') + _ptr('stream')),
    'rsa_eimn_dffm_workspace_bytes': (C.c_int64, _i32('batch', 'H', 'W', 'C')),
    'rsa_eimn_dffm_reduce': (C.c_int, _ptr('z') + _i32('batch', 'H', 'W', 'C') + _ptr('gamma', 'beta') + _f32('eps') + _ptr('workspace') + _i64('workspace_bytes') + _ptr('stream')),
    'rsa_eimn_dffm_gates': (C.c_int, _ptr('workspace') + _i64('workspace_bytes') + _i32('batch', 'H', 'W', 'C', 'rc') + _ptr('wg', 'bg', 'wc', 'bc', 'ws', 'bs', 'gates', 'stream')),
    'rsa_eimn_dffm_apply': (C.c_int, _ptr('z', 'x') + _i32('batch', 'H', 'W', 'C', 'rc') + _ptr('gamma', 'beta') + _f32('eps') + _ptr('wl', 'bl', 'ws', 'gates', 'scale', 'norm_gamma', 'norm_beta') + _f32('norm_eps') + _ptr('add', 'out_f32') + _plane_fields('out') + _i32('fmt') + _ptr('stream')),
    'rsa_rha_window_attn_lds_bytes': (C.c_int64, _i32('C2', 'window')),
    'rsa_rha_window_attn': (C.c_int, _plane_fields('x') + _i32('batch', 'H', 'W', 'C2', 'down', 'window', 'shift', 'fmt') + _ptr('wqkv_t', 'bqkv', 'pos_t', 'inv_scale', 'dwc_w', 'dwc_b', 'wproj_t', 'bproj', 'out', 'stream')),
    'rsa_rha_mix': (C.c_int, _plane_fields('x') + _ptr('att') + _plane_fields('out') + _i32('batch', 'H', 'W', 'C2', 'down', 'fmt') + _ptr('weight', 'bias', 'stream')),
    'rsa_rha_gate': (C.c_int, _plane_fields('f') + _plane_fields('a') + _plane_fields('out') + _i32('batch', 'H', 'W', 'hidden_planes', 'i_planes', 'fmt') + _ptr('stream')),
    'rsa_flex_norm_shift': (C.c_int, _ptr('x_f32') + _i32('batch', 'H', 'W', 'C') + _f32('eps') + _ptr('norm_weight', 'weight') + _plane_fields('out') + _i32('fmt') + _ptr('stream')),
    'rsa_flex_window_attn_lds_bytes': (C.c_int64, _i32('C', 'products')),
    'rsa_flex_window_attn': (C.c_int, _plane_fields('qkv') + _plane_fields('out') + _i32('batch', 'H', 'W', 'C', 'products', 'fmt') + _ptr('lepe_w', 'lepe_b', 'stream')),
    'rsa_flex_sqrelu': (C.c_int, _plane_fields('in') + _plane_fields('out') + _i32('batch', 'H', 'W', 'hidden', 'norm') + _f32('eps') + _i32('fmt') + _ptr('stream')),
    'rsa_flex_gate_add': (C.c_int, _plane_fields('r') + _plane_fields('kv') + _ptr('base_f32', 'out_f32') + _plane_fields('out') + _i32('batch', 'H', 'W', 'C', 'fmt') + _ptr('stream')),
    'rsa_version': (C.c_int, []),
    'rsa_last_error_string': (C.c_char_p, []),
}

EXPORTS = tuple(SIGNATURES)  # every symbol the header declares

# Entry points of the same library that a header of their own declares beside include/resselt_amd.h (include/resselt_amd_<family>.h), with
# their mirrors and rows in an engine/lib_<family>.py: name -> row, as in SIGNATURES.  ``extend`` adds them; ``load`` demands and types them
# like the rows above, and ``launch`` / ``invoke`` reach them by name.
EXTENSIONS: dict = {}

# Every header under include/ -> the rows table that mirrors it, extensions in registration order (tests/test_capi_headers.py compares
# each table, and the mirrors of the module that holds it, with its header).
HEADERS: dict = {'resselt_amd.h': SIGNATURES}

# Entry points of the library that no header under include/ declares: helpers of the engine's plan builder and of its tiler, documented
# where csrc/ defines them (capi.hip, tile_blend.hip, resample.hip, yuv.hip, rgba.hip).  Rows as in SIGNATURES; ``load`` demands and types them like the rest.
INTERNAL = {
    'rsa_conv2d_list_assign_tile_order': (C.c_int, _conv('list') + _i32('n', 'first_order') + [('next_order', C.POINTER(C.c_int32))]),
    # the tiler's seam blending (csrc/tile_blend.hip documents the arguments)
    'rsa_tile_blend_accumulate': (C.c_int, _ptr('src') + _i32('src_dtype', 'batch', 'C', 'win_h', 'win_w', 'src_h', 'src_w', 'src_y', 'src_x') + _ptr('acc') + _i32('acc_h', 'acc_w', 'acc_y', 'acc_x', 'ramp_top', 'ramp_bottom', 'ramp_left', 'ramp_right') + _ptr('stream')),
    # upscale(out_size=): the native frame at any size, one launch (csrc/resample.hip documents the arguments)
    'rsa_resample': (C.c_int, _ptr('src') + _i32('src_dtype', 'batch', 'C', 'src_h', 'src_w') + _ptr('dst') + _i32('dst_dtype', 'dst_h', 'dst_w') + _ptr('start_y', 'weight_y') + _i32('taps_y') + _ptr('start_x', 'weight_x') + _i32('taps_x') + _ptr('stream')),
    # upscale_yuv(): NV12 / P010 planes <-> float NCHW (csrc/yuv.hip documents the arguments)
    'rsa_yuv420_to_nchw': (C.c_int, _ptr('y') + _i64('y_pitch', 'y_batch_stride') + _ptr('uv') + _i64('uv_pitch', 'uv_batch_stride') + _i32('bits', 'batch', 'H', 'W', 'matrix', 'full_range', 'chroma_loc') + _ptr('dst') + _i32('dst_dtype') + _ptr('stream')),
    'rsa_nchw_to_yuv420': (C.c_int, _ptr('src') + _i32('src_dtype', 'batch', 'H', 'W', 'matrix', 'full_range', 'chroma_loc', 'bits') + _ptr('y') + _i64('y_pitch', 'y_batch_stride') + _ptr('uv') + _i64('uv_pitch', 'uv_batch_stride') + _ptr('stream')),
    # upscale_rgba(): interleaved gray / gray + alpha / RGB / RGBA images of 8 or 16 bits <-> float NCHW (csrc/rgba.hip documents the arguments)
    'rsa_image_to_nchw_alpha': (C.c_int, _ptr('img') + _i64('pitch', 'batch_stride') + _i32('bits', 'batch', 'H', 'W', 'C', 'Cm', 'bleed') + _ptr('color') + _i32('color_dtype') + _ptr('alpha') + _i32('alpha_mode') + _ptr('flags', 'stream')),
    'rsa_nchw_to_image_alpha': (C.c_int, _ptr('color') + _i32('color_dtype', 'Cm') + _ptr('alpha') + _i32('alpha_dtype', 'Ca', 'batch', 'H', 'W', 'C', 'bits') + _ptr('img') + _i64('pitch', 'batch_stride') + _ptr('stream')),
}


def _declare(lib, rows: dict) -> None:
    for name, (restype, params) in rows.items():
        if not hasattr(lib, name):
            raise RuntimeError(f'{lib_path()} does not export {name}; rebuild the library')
        getattr(lib, name).argtypes = [ctype for _, ctype in params]
        getattr(lib, name).restype = restype


def extend(rows: dict, header: str) -> None:
    """Register the signature rows of extension header ``header`` (its file name under include/; once, at the import of its
    engine/lib_<family>.py).  A name that another header's table already holds raises ``ValueError``, and nothing is registered."""
    owner = {name: h for h, table in HEADERS.items() if h != header for name in table}
    clash = [name for name in rows if name in owner]
    if clash:
        raise ValueError(f'{clash} are entry points of include/{owner[clash[0]]}')
    HEADERS[header] = rows
    EXTENSIONS.update(rows)
    if _lib is not None:
        _declare(_lib, rows)


def lib_path() -> str:
    """The in-tree library; RSA_LIB=path selects an experiment build instead (tools/variant.sh: A/B timing, ablations)."""
    override = os.environ.get('RSA_LIB')
    if override:
        return os.path.abspath(override)
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), _LIB_NAME)


def _warn_if_stale(path: str) -> None:
    """The build stamps the library with the hash of the sources it was built from (build.py); a library that no longer matches the
    sources next to it still loads (the GPU box only has the prebuilt file), but says so."""
    try:
        from .. import build as B

        if os.path.abspath(path) != os.path.abspath(B.OUT) or not os.path.isdir(B.CSRC):
            return
        have = None
        if os.path.exists(B.STAMP):
            with open(B.STAMP) as f:
                have = f.read().strip()
        if have != B._hash():
            import warnings

            warnings.warn(f'{_LIB_NAME} was built from other sources than the ones in {B.CSRC} (stamp {str(have)[:12]}); run `python -m resselt_amd.build`', RuntimeWarning, stacklevel=3)
    except OSError:
        pass


def load() -> C.CDLL:
    """Load the HIP library once; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f'{_LIB_NAME} not found at {path}: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950). resselt_amd has no CPU fallback.'
        )
    _warn_if_stale(path)
    lib = C.CDLL(path)
    for rows in HEADERS.values():
        _declare(lib, rows)
    _declare(lib, INTERNAL)
    _lib = lib
    return lib


class Fp16RangeError(RuntimeError):
    """``rsa_check_status`` after ``rsa_check_finite`` met an infinity or a NaN: an activation of a one-product fp16 layer left the
    format's range (or the input was not finite).  ``precision = 'auto'`` answers it by re-running in three bf16 products."""


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().rsa_last_error_string()
        cls = Fp16RangeError if rc == E_FP16_RANGE else RuntimeError
        raise cls(f'{what} failed (status {rc}): {msg.decode() if msg else "?"}')


def signature(name: str) -> tuple:
    """The row of entry point ``name``: of include/resselt_amd.h or of an extension header."""
    return SIGNATURES[name] if name in SIGNATURES else EXTENSIONS[name]


def bind(name: str, **kwargs) -> list:
    """Resolve keyword arguments against ``SIGNATURES[name]`` (or the row of an extension header, ``EXTENSIONS[name]``) into the positional argument list of the entry point, without its trailing
    stream.  Keys are the header's parameter names (a trailing underscore is dropped: ``in_``).  Values:

    ``Planes`` / ``PlaneRows`` under key ``k`` fill ``k_hi``, ``k_lo``, ``k_plane_stride`` and ``k_batch_stride`` (``(planes, plane0)`` from
    that plane on, as in ``ops.conv_params(res1=...)``); an explicit ``k_lo=`` beside it replaces the lo pointer (``None`` for a reader that
    must not see lo halves).  A tensor becomes its ``data_ptr()``, ``None`` becomes NULL, numbers and descriptors pass through.
    A missing, unknown or doubly given parameter raises ``TypeError``: nothing has been launched by then."""
    params = [k for k, _ in signature(name)[1]]
    given = {'stream': None} if params and params[-1] == 'stream' else {}  # the caller of the entry point supplies it

    def put(key, value, replace=False):
        if key not in params:
            raise TypeError(f'{name}: no parameter {key!r}')
        if key in given and not replace:
            raise TypeError(f'{name}: parameter {key!r} given twice')
        given[key] = value

    scalars = {}
    for key, v in kwargs.items():
        key = key[:-1] if key.endswith('_') else key
        v, plane0 = v if isinstance(v, tuple) else (v, 0)
        if hasattr(v, 'hi_ptr'):
            put(f'{key}_hi', v.hi_ptr(plane0))
            put(f'{key}_lo', v.lo_ptr(plane0))
            put(f'{key}_plane_stride', v.plane_stride)
            put(f'{key}_batch_stride', v.batch_stride)
        elif plane0:
            raise TypeError(f'{name}: {key!r} has a plane offset but is no plane buffer')
        else:
            scalars[key] = v.data_ptr() if hasattr(v, 'data_ptr') else v
    for key, v in scalars.items():
        put(key, v, replace=key.endswith('_lo') and key in given)
    missing = [k for k in params if k not in given]
    if missing:
        raise TypeError(f'{name}: missing parameter {", ".join(map(repr, missing))}')
    return [given[k] for k in params if k != 'stream']


def invoke(name: str, args, stream: int) -> None:
    """Call entry point ``name`` with the positional ``args`` of ``bind`` on ``stream`` and raise if it fails."""
    check(getattr(load(), name)(*args, stream), name)


def call(name: str, stream: int, **kwargs) -> None:
    """One immediate C-ABI call by parameter name (see ``bind``) on ``stream``; raises if it fails."""
    invoke(name, bind(name, **kwargs), stream)


def launch(name: str, params, stream: int) -> None:
    """Call the C-ABI entry point ``name`` that takes ``(params*, stream)`` and raise if it fails."""
    invoke(name, [params], stream)


def check_finite(t, stream: int) -> None:
    """Scan a plain float tensor (or the hi / lo storage of a split-plane buffer) for non-finite values (``rsa_check_finite``; asynchronous:
    ``check_status`` raises ``Fp16RangeError`` once the launch has completed)."""
    import torch

    dt = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}[t.dtype]
    if not t.is_contiguous():
        raise ValueError('check_finite: the tensor must be contiguous')
    call('rsa_check_finite', stream, data=t, dtype=dt, count=t.numel())


def conv2d_list(params: 'C.Array[ConvParams] | list[ConvParams]', stream: int) -> None:
    """Launch a list of fused convolutions in order on ``stream`` with one host call."""
    arr = (ConvParams * len(params))(*params) if isinstance(params, list) else params
    invoke('rsa_conv2d_list', [arr, len(arr)], stream)


def conv_kernel_name(p: ConvParams) -> str:
    return load().rsa_conv_kernel_name(C.byref(p)).decode()


def ring_aborts() -> int:
    return int(load().rsa_debug_ring_aborts())


def check_status(what: str = 'forward') -> None:
    """Raise when a ring-schedule kernel of a COMPLETED launch reported a failed hand-off (``rsa_check_status``: reads a host-visible word,
    never synchronises).  Synchronise the stream first to judge the launches still in flight."""
    check(load().rsa_check_status(), f'{what}: rsa_check_status')


def conv2d_pair(a: ConvParams, b: ConvParams, stream: int) -> None:
    """Two consecutive growth convolutions of a residual dense block as ONE launch (``rsa_conv2d_pair``; csrc/conv_ring_pair.h)."""
    call('rsa_conv2d_pair', stream, a=a, b=b)


def conv_pair_fusable(a: ConvParams, b: ConvParams) -> bool:
    return bool(load().rsa_conv_pair_fusable(C.byref(a), C.byref(b)))


def conv_list_assign_tile_order(arr: 'C.Array[ConvParams]', first_order: int) -> int:
    """Serpentine order per LAUNCH (``rsa_conv2d_list_assign_tile_order``; host only, nothing is launched): launch k of what
    ``rsa_conv2d_list`` makes of ``arr`` gets ``tile_order = (first_order + k) & 1``, both halves of a fused pair the pair's.  Returns the
    order the launch behind the list would get (the ``first_order`` of the next list of the same forward)."""
    nxt = C.c_int32(0)
    check(load().rsa_conv2d_list_assign_tile_order(arr, len(arr), first_order, C.byref(nxt)), 'rsa_conv2d_list_assign_tile_order')
    return int(nxt.value)


def tile_blend_accumulate(src: int, src_dtype: int, batch: int, channels: int, window: tuple, src_size: tuple, src_offset: tuple,
                          acc: int, acc_size: tuple, acc_offset: tuple, ramps: tuple, stream: int) -> None:
    """Add one tile's weighted window into the full-frame f32 accumulator (``rsa_tile_blend_accumulate``, csrc/tile_blend.hip).  ``src`` /
    ``acc``: device addresses; ``window``, the sizes and the offsets are ``(rows, columns)`` in output pixels; ``ramps`` = widths of the
    ``(top, bottom, left, right)`` ramps."""
    check(load().rsa_tile_blend_accumulate(src, src_dtype, batch, channels, *window, *src_size, *src_offset, acc, *acc_size, *acc_offset, *ramps, stream),
          'rsa_tile_blend_accumulate')  # fmt: skip


def resample(src: int, src_dtype: int, batch: int, channels: int, src_size: tuple, dst: int, dst_dtype: int, dst_size: tuple,
             table_y: tuple, table_x: tuple, stream: int) -> None:
    """Resample a dense frame to ``dst_size`` in one launch (``rsa_resample``, csrc/resample.hip).  ``src`` / ``dst``: device addresses;
    the sizes are ``(rows, columns)``; ``table_y`` / ``table_x`` = ``(start address, weight address, taps)`` of the device copies of
    ``tiling.resample_table`` for the rows and the columns."""
    check(load().rsa_resample(src, src_dtype, batch, channels, *src_size, dst, dst_dtype, *dst_size, *table_y, *table_x, stream), 'rsa_resample')


def yuv420_to_nchw(y: tuple, uv: tuple, bits: int, batch: int, size: tuple, matrix: int, full_range: int, chroma_loc: int, dst: int, dst_dtype: int,
                   stream: int) -> None:
    """NV12 (``bits = 8``) / P010 (``bits = 10``) planes -> dense float ``[batch, 3, H, W]`` in one launch (``rsa_yuv420_to_nchw``,
    csrc/yuv.hip).  ``y`` / ``uv`` = ``(device address, pitch, batch stride)`` in bytes; ``size = (H, W)`` of the luma plane; ``matrix``,
    ``full_range`` and ``chroma_loc`` are the integers of ``ops.YUV_MATRICES`` / ``YUV_RANGES`` / ``YUV_CHROMA_LOCS``."""
    check(load().rsa_yuv420_to_nchw(*y, *uv, bits, batch, *size, matrix, full_range, chroma_loc, dst, dst_dtype, stream), 'rsa_yuv420_to_nchw')


def nchw_to_yuv420(src: int, src_dtype: int, batch: int, size: tuple, matrix: int, full_range: int, chroma_loc: int, bits: int, y: tuple, uv: tuple,
                   stream: int) -> None:
    """Dense float ``[batch, 3, H, W]`` -> NV12 / P010 planes in one launch (``rsa_nchw_to_yuv420``, csrc/yuv.hip); arguments as
    ``yuv420_to_nchw``."""
    check(load().rsa_nchw_to_yuv420(src, src_dtype, batch, *size, matrix, full_range, chroma_loc, bits, *y, *uv, stream), 'rsa_nchw_to_yuv420')


def image_to_nchw_alpha(img: tuple, bits: int, batch: int, size: tuple, channels: int, model_channels: int, bleed: int, color: int, color_dtype: int,
                        alpha: int | None, alpha_mode: int, flags: int | None, stream: int) -> None:
    """An interleaved 8- / 16-bit image of 1 .. 4 channels -> the dense float ``[batch, model_channels, H, W]`` colour tensor (edge-bled under
    transparent pixels), the alpha tensor and the per-image "some alpha is below the maximum" flags in one launch
    (``rsa_image_to_nchw_alpha``, csrc/rgba.hip).  ``img`` = ``(device address, pitch, batch stride)`` in bytes; ``size = (H, W)``;
    ``alpha_mode``: 0 none, 1 replicated in ``color_dtype``, 2 one f32 channel; ``flags``: zeroed int32 ``[batch]``."""
    check(load().rsa_image_to_nchw_alpha(*img, bits, batch, *size, channels, model_channels, bleed, color, color_dtype, alpha, alpha_mode, flags, stream),
          'rsa_image_to_nchw_alpha')  # fmt: skip


def nchw_to_image_alpha(color: int, color_dtype: int, model_channels: int, alpha: int | None, alpha_dtype: int, alpha_channels: int, batch: int,
                        size: tuple, channels: int, bits: int, img: tuple, stream: int) -> None:
    """Dense float colour ``[batch, model_channels, H, W]`` and an optional alpha source ``[batch, alpha_channels, H, W]`` -> the interleaved
    8- / 16-bit image of ``channels`` in one launch (``rsa_nchw_to_image_alpha``, csrc/rgba.hip); arguments as ``image_to_nchw_alpha``."""
    check(load().rsa_nchw_to_image_alpha(color, color_dtype, model_channels, alpha, alpha_dtype, alpha_channels, batch, *size, channels, bits, *img, stream),
          'rsa_nchw_to_image_alpha')  # fmt: skip


def set_pair_fusion(mode: int) -> None:
    """Debug / A-B: 1 = ``rsa_conv2d_list`` fuses eligible neighbours, 0 = it launches them one by one, -1 = follow RSA_CONV_PAIR."""
    load().rsa_debug_set_pair(int(mode))


def set_ring_spin_limit(polls: int) -> None:
    load().rsa_debug_set_ring_spin_limit(int(polls))


def cout_tiles(cout: int) -> int:
    return int(load().rsa_conv_cout_tiles(cout))
