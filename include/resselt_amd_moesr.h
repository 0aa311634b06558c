/*
 * resselt_amd_moesr.h — the MoESR entry point of libresselt_amd.so, an extension of the C-ABI in resselt_amd.h (same conventions, same
 * library): the reference's archs/moesr/arch.py; resselt_amd/csrc/moesr.hip.  Its ctypes mirror and signature row live in
 * resselt_amd/engine/lib_moesr.py, and tests/test_moesr_capi.py compares the two field by field and argument by argument, as
 * tests/test_pack_and_capi.py and tests/test_capi_signatures.py do for resselt_amd.h.
 */
#ifndef RESSELT_AMD_MOESR_H
#define RESSELT_AMD_MOESR_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The f32 residual stream of MoESR between its convolutions: one pass gathers the next stream value s_out of every pixel and writes it as
 * an f32 map and / or as split planes, the planes either normalised for the next gated block or plain for the next convolution.
 * H x W is the size of the OUTPUT stream, C = dim its channel count: a multiple of 8 from 8 to 128 (the range of MoSR's _check_dims; a
 * lane keeps all C channels of its pixel in registers).  Every f32 map is NCHW4c [N][ceil(channels/4)][h][w][4].
 *   mode 0, block tail (GatedCNNBlock.forward :163-164):  a = fc2 + Mish, C channels at H x W;
 *       s_out[c] = a[c] * gamma[c] + s_in[c]
 *   mode 1, MSG entry (MSG.down :170):  a = the down-convolution, C/4 channels at a_H x a_W = 2H x 2W, its LeakyReLU already applied (it
 *       commutes with the permutation); C/4 need not be a multiple of 4;
 *       s_out[c] = a[c / 4][2y + (c % 4) / 2][2x + c % 2]                                       (PixelUnshuffle(2))
 *   mode 2, MSG exit (MSG.up, MSG.forward :172-177, MoESR.forward :225):  a = the up-convolution, 4C channels at a_H x a_W = H/2 x W/2,
 *       LeakyReLU applied;
 *       s_out[c] = a[4c + 2(y % 2) + x % 2][y / 2][x / 2] + s_in[c] (+ s2_in[c])                (PixelShuffle(2) + x, + the trunk residual)
 * Outputs, each optional, at least one: s_out as an f32 map (may equal s_in), and split planes [N][C/8][H][W][8] of format fmt (out_lo may
 * be NULL).  With ln_gamma the planes hold LayerNorm over the channels of s_out (centred form, eps > 0, ln_gamma / ln_beta [C]); with
 * ln_gamma NULL they hold s_out itself.  C % 8 == 0, so a last plane has no tail channels; were there any they would be written as zero.
 * Errors: RSA_E_ARG for a null required pointer, bad geometry (C, mode, a_H / a_W not the size the mode reads: in particular an odd
 * source size in mode 1 and an odd stream size in mode 2), RSA_E_ALIGN for a pointer that is not 16-byte aligned. */
typedef struct rsa_moesr_stream_params {
  int32_t batch;
  int32_t H, W;              /* the output stream */
  int32_t C;                 /* dim: 8..128, a multiple of 8 */
  int32_t mode;              /* 0, 1 or 2 */
  int32_t a_H, a_W;          /* size of a: H x W (mode 0), 2H x 2W (mode 1), H/2 x W/2 (mode 2) */
  int32_t fmt;               /* enum rsa_plane_fmt of out_hi / out_lo */
  const float* a;
  const float* gamma;        /* mode 0: [C] */
  const float* s_in;         /* modes 0 and 2 */
  const float* s2_in;        /* mode 2, may be NULL */
  float* s_out;              /* may be NULL */
  const float* ln_gamma;     /* [C]; NULL: plain planes */
  const float* ln_beta;      /* [C], with ln_gamma */
  float eps;                 /* with ln_gamma */
  int32_t reserved0;         /* must be 0 */
  void* out_hi;              /* may be NULL */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;  /* 16-byte units, >= H*W */
  int64_t out_batch_stride;
} rsa_moesr_stream_params;
int rsa_moesr_stream(const rsa_moesr_stream_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_MOESR_H */
