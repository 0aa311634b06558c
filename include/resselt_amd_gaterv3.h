/*
 * resselt_amd_gaterv3.h — the entry points GateRV3 adds to libresselt_amd.so, an extension of the C-ABI in resselt_amd.h (same conventions,
 * same library): the reference's archs/gaterv3/arch.py; resselt_amd/csrc/gaterv3.hip.  The ctypes mirrors and signature rows live in
 * resselt_amd/engine/lib_gaterv3.py, and tests/test_gaterv3_capi.py compares the two field by field.
 *
 * Conventions: split planes [N][planes][H][W][8] of `fmt` (enum rsa_plane_fmt), the lo plane optional; f32 stream maps [N][C/4][H][W][4];
 * all arithmetic in f32; no atomics; every reduction runs in a fixed order that depends on (H, W) alone, so a result is bit-identical
 * from run to run.
 */
#ifndef RESSELT_AMD_GATERV3_H
#define RESSELT_AMD_GATERV3_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reduction chunk of rsa_gaterv3_local_gate: one tile of RSA_GATERV3_TILE_W x RSA_GATERV3_TILE_H pixels (tiles in row-major order
 * from the top left of the map; a tile at the right / bottom edge is partly outside and sums the pixels inside). */
#define RSA_GATERV3_TILE_W 32
#define RSA_GATERV3_TILE_H 8
/* The token chunk of rsa_gaterv3_channel_attention's partial sums: consecutive tokens (pixels in row-major order). */
#define RSA_GATERV3_TOKEN_CHUNK 128

/* MetaGated.local's grouped 3x3 + SimpleGate (gaterv3/arch.py:642-643) and the pooling of `sca` (:645-646), one launch.
 *   conv[o] = bias[o] + sum_{i < 2, ky, kx} weight[o][i][ky][kx] * x[2 floor(o / 2) + i][y + ky - 1][x + kx - 1]      (zero padding 1)
 *             an f32 fma chain from the bias in the order i, ky, kx;      o < 2 dim
 *   s[c]    = conv[c] * conv[dim + c]                                     c < dim, written as dim / 8 split planes
 *   workspace[n][tile][c] = sum of s[c] (the f32 value, before it is rounded to planes) over the pixels of the tile that lie in the map
 * x: the 2 dim / 8 planes of local.1's output (plane p of s reads planes p and p + dim / 8: group pairs never straddle a plane).
 * weight f32 [2 dim][2][9], bias f32 [2 dim].  x and out must not overlap.  Each halo tile of x is read from memory once per launch and
 * staged in LDS as f32.  workspace: rsa_gaterv3_local_workspace_bytes(batch, H, W, dim) bytes, 16-byte aligned; the same buffer goes
 * to rsa_gaterv3_sca_apply.
 * Errors: RSA_E_ARG null pointer / bad geometry / bad fmt / reserved field / workspace too small / x and out overlap;
 * RSA_E_UNSUPPORTED dim not a multiple of 8 or above 512; RSA_E_ALIGN. */
typedef struct rsa_gaterv3_local_gate_params {
  int32_t batch;
  int32_t H, W;
  int32_t dim;                 /* multiple of 8, 8..512 */
  int32_t fmt;                 /* enum rsa_plane_fmt of x and out */
  int32_t reserved0;           /* must be 0 */
  const void* x_hi;
  const void* x_lo;            /* may be NULL */
  int64_t x_plane_stride;      /* 16-byte units */
  int64_t x_batch_stride;
  const float* weight;
  const float* bias;
  void* out_hi;
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  float* workspace;
  int64_t workspace_bytes;
} rsa_gaterv3_local_gate_params;
int64_t rsa_gaterv3_local_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t dim); /* <= 0: geometry refused */
int rsa_gaterv3_local_gate(const rsa_gaterv3_local_gate_params* p, void* stream);

/* `x * sca(x) * gamma0 + short` (gaterv3/arch.py:664-665) from rsa_gaterv3_local_gate's outputs.  TWO kernels in one call:
 *   1. one workgroup per image: mean[c] = (sum of the tile sums) / (H W) -- K = 256 / dim consecutive runs of ceil(tiles / K) tiles, each
 *      added in ascending tile order, then the K run sums in ascending order (K = 1 above 256 channels) --, then
 *      a[n][o] = gamma0[o] * (sca_b[o] + sum_c sca_w[o][c] * mean[c])  (an fma chain from the bias, ascending c), kept in the workspace;
 *   2. out = s * a + short on f32 stream maps, one fma per value.
 * s: the dim / 8 planes rsa_gaterv3_local_gate wrote; sca_w f32 [dim][dim] ([output][input]), sca_b, gamma0 f32 [dim]; short_f32 and
 * out_f32 [N][dim/4][H][W][4] (out may be short).
 * Errors: as rsa_gaterv3_local_gate. */
typedef struct rsa_gaterv3_sca_apply_params {
  int32_t batch;
  int32_t H, W;
  int32_t dim;
  int32_t fmt;                 /* enum rsa_plane_fmt of s */
  int32_t reserved0;           /* must be 0 */
  const void* s_hi;
  const void* s_lo;            /* may be NULL */
  int64_t s_plane_stride;
  int64_t s_batch_stride;
  const float* sca_w;
  const float* sca_b;
  const float* gamma0;
  const float* short_f32;
  float* out_f32;
  float* workspace;
  int64_t workspace_bytes;
} rsa_gaterv3_sca_apply_params;
int rsa_gaterv3_sca_apply(const rsa_gaterv3_sca_apply_params* p, void* stream);

/* The latent Attention (gaterv3/arch.py:549-584; Restormer's transposed attention) behind qkv_dwconv, per image and head over ALL
 * tokens t < H W.  Head h owns channels [h d, (h + 1) d) of q, of k and of v wherever they fall in the planes.
 *   G[i][j] = sum_t q_i[t] k_j[t],   |q_i|^2 = sum_t q_i[t]^2,   |k_j|^2 likewise
 *   A[i][:] = softmax_j(temperature[h] * G[i][j] / (max(|q_i|, 1e-12) * max(|k_j|, 1e-12)))          the row maximum subtracted
 *   out_i[t] = sum_j A[i][j] v_j[t]                                                                  an fma chain from 0, ascending j
 * THREE kernels in one call: partial sums of G and of the squared norms per chunk of RSA_GATERV3_TOKEN_CHUNK consecutive tokens (an fma
 * chain from 0 in ascending token order); one ordered finish per (image, head) that adds the partial records in ascending chunk order and
 * forms A; the apply pass.  qkv: 3 C / 8 planes [q | k | v]; out: C / 8 planes; they must not overlap.  temperature f32 [heads].
 * Errors: RSA_E_ARG null pointer / bad geometry / bad fmt / reserved field / heads * head_dim != C / workspace too small / overlap;
 * RSA_E_UNSUPPORTED C not a multiple of 8, heads outside 1..16, head_dim outside 1..64; RSA_E_ALIGN. */
typedef struct rsa_gaterv3_attn_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                   /* multiple of 8 */
  int32_t heads;               /* 1..16 */
  int32_t head_dim;            /* 1..64, heads * head_dim == C */
  int32_t fmt;                 /* enum rsa_plane_fmt of qkv and out */
  int32_t reserved0;           /* must be 0 */
  const void* qkv_hi;
  const void* qkv_lo;          /* may be NULL */
  int64_t qkv_plane_stride;
  int64_t qkv_batch_stride;
  const float* temperature;
  void* out_hi;
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  float* workspace;
  int64_t workspace_bytes;
} rsa_gaterv3_attn_params;
int64_t rsa_gaterv3_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t heads, int32_t head_dim); /* <= 0: refused */
int rsa_gaterv3_channel_attention(const rsa_gaterv3_attn_params* p, void* stream);

/* `+ gamma * nn.Upsample(scale)(inp)` on the cropped output (gaterv3/arch.py:801-802):
 *   out[n][c][Y][X] = round(out[n][c][Y][X] + round(gamma[c] * x[n][c][Y / scale][X / scale]))        Y < h scale, X < w scale
 * with both roundings in `dtype` (the product and the sum are separate operations, as torch's are).  x is the caller's UNPADDED
 * [N][C][h][w] tensor, out [N][C][out_H][out_W] with out_H >= h scale and out_W >= w scale (the padded part is not touched), both of
 * `dtype` (RSA_F32 / RSA_F16 / RSA_BF16); gamma f32 [C].
 * Errors: RSA_E_ARG null pointer / bad geometry / out smaller than the scaled input / reserved field; RSA_E_UNSUPPORTED dtype. */
typedef struct rsa_gaterv3_shortcut_params {
  int32_t batch;
  int32_t C;
  int32_t h, w;                /* of x */
  int32_t scale;               /* 1..8 */
  int32_t out_H, out_W;
  int32_t dtype;               /* enum rsa_dtype */
  const void* x;
  const float* gamma;
  void* out;
} rsa_gaterv3_shortcut_params;
int rsa_gaterv3_shortcut(const rsa_gaterv3_shortcut_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_GATERV3_H */
