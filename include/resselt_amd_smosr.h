/*
 * resselt_amd_smosr.h — the SMoSR entry points of libresselt_amd.so, an extension of the C-ABI in resselt_amd.h (same conventions, same
 * library): the reference's archs/smosr/arch.py; resselt_amd/csrc/smosr.hip.  Their ctypes mirrors and signature rows live in
 * resselt_amd/engine/lib_smosr.py, and tests/test_smosr_capi.py compares the two field by field and argument by argument, as
 * tests/test_moesr_capi.py does for resselt_amd_moesr.h.
 */
#ifndef RESSELT_AMD_SMOSR_H
#define RESSELT_AMD_SMOSR_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tail of an SMB (SMB.forward :413-415): a = body.4's f32 map, 2C channels at H x W (value half [0, C), gate half [C, 2C));
 *     v[c] = (a[c] + s_in[c]) * tanh(a[C + c]) (+ s2_in[c])
 * with the device library's tanhf.  s_in is the block's shortcut (the previous stream, or the f32 map of the 1x1 `short` convolution),
 * s2_in the trunk residual behind the last block of blocks_2 (may be NULL).  Every f32 map is NCHW4c [N][ceil(channels/4)][H][W][4].
 * Outputs, each optional, at least one: s_out, the f32 stream of C channels (may equal s_in or s2_in: a lane reads its pixel before it
 * writes it), and split planes [N][C/8][H][W][8] of format fmt holding v (out_lo may be NULL).  C: a multiple of 8 from 8 to 128.
 * Errors: RSA_E_ARG for a null required pointer, bad geometry or format, no output, s_out == a (the two maps have different batch
 * strides: not an in-place form), a plane stride below H*W; RSA_E_ALIGN for a pointer that is not 16-byte aligned. */
typedef struct rsa_smosr_gate_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                 /* 8..128, a multiple of 8 */
  int32_t fmt;               /* enum rsa_plane_fmt of out_hi / out_lo */
  int32_t reserved0;         /* must be 0 */
  const float* a;            /* 2C channels */
  const float* s_in;
  const float* s2_in;        /* may be NULL */
  float* s_out;              /* may be NULL */
  void* out_hi;              /* may be NULL */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;  /* 16-byte units, >= H*W */
  int64_t out_batch_stride;
} rsa_smosr_gate_params;
int rsa_smosr_gate(const rsa_smosr_gate_params* p, void* stream);

/* The front end (SMoSR.forward :452): a plain [N][C][src_h][src_w] tensor of `dtype` (enum rsa_dtype: f32, f16 or bf16) -> split planes
 * [N][ceil(C/8)][src_h + 2 pad][src_w + 2 pad][8] with F.pad(x, (pad, pad, pad, pad), 'reflect') fused into the read; tail channels are
 * written as zero.  The values are those rsa_nchw_to_planes writes for the padded tensor, bit for bit.
 * Errors: RSA_E_ARG for a null pointer, bad geometry, pad < 0 or pad >= src_h or src_w (the reflection needs pad + 1 pixels), a bad dtype
 * or format, a plane stride below the padded map; RSA_E_ALIGN for planes that are not 16-byte aligned. */
typedef struct rsa_smosr_pad_params {
  int32_t batch;
  int32_t C;
  int32_t src_h, src_w;
  int32_t pad;
  int32_t dtype;             /* enum rsa_dtype of x */
  int32_t fmt;               /* enum rsa_plane_fmt of out_hi / out_lo */
  int32_t reserved0;         /* must be 0 */
  const void* x;
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;  /* 16-byte units, >= (src_h + 2 pad) * (src_w + 2 pad) */
  int64_t out_batch_stride;
} rsa_smosr_pad_params;
int rsa_smosr_pad(const rsa_smosr_pad_params* p, void* stream);

/* Pixel attention with the LeakyReLU behind it (PA.forward :83-84, UniUpsampleV4_light :146-147), planes to planes in one pass:
 *     y = leaky_relu(x * sigmoid(W x + b), slope),   W [C][C] a 1x1 convolution, x = in_hi (+ in_lo)
 * C: a multiple of 8 from 8 to 128; K = ceil(C / 32) chunks of 32 channels.  The product runs on v_mfma_f32_16x16x32 of format fmt:
 * products = 1 multiplies the hi halves, products = 3 adds W_lo x_hi and W_hi x_lo (in_lo required).
 * w_frag: the weights as A fragments, 16-bit values of format fmt, [K out chunks][K in chunks][2 tiles][products == 3 ? 2 : 1 halves]
 * [64 lanes][8]: lane l of tile t of (out chunk mo, in chunk k) holds W[32 mo + 8 ((l & 15) >> 2) + 4 t + (l & 3)][32 k + 8 (l >> 4) + j],
 * j = 0..7, zero past C, so that the two accumulators of a lane are the 8 channels of one plane unit: the unit it loaded as its B
 * fragment.  bias: f32 [32 K], zero past C.  Both are what resselt_amd/engine/lib_smosr.py: pack_pa_weights builds.
 * The image is a run of H*W pixels: no size is special, and no buffer needs padding.  In place (out_hi == in_hi, out_lo == in_lo) is
 * allowed with equal strides.
 * Errors: RSA_E_ARG for a null required pointer, bad geometry, format or products, in_lo missing for three products, a plane stride
 * below H*W, an in-place call with different strides or with out_lo != in_lo; RSA_E_ALIGN for a pointer that is not 16-byte aligned. */
typedef struct rsa_smosr_pa_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                 /* 8..128, a multiple of 8 */
  int32_t fmt;               /* enum rsa_plane_fmt of every plane operand and of w_frag */
  int32_t products;          /* 1 or 3 */
  float slope;               /* of the LeakyReLU (1 = none) */
  int32_t reserved0;         /* must be 0 */
  const void* w_frag;
  const float* bias;
  const void* in_hi;
  const void* in_lo;         /* may be NULL with products == 1 */
  int64_t in_plane_stride;   /* 16-byte units, >= H*W */
  int64_t in_batch_stride;
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_smosr_pa_params;
int rsa_smosr_pa(const rsa_smosr_pa_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_SMOSR_H */
