/*
 * resselt_amd_gaterv2.h — the entry point GateRv2 adds to libresselt_amd.so, an extension of the C-ABI in resselt_amd.h (same conventions,
 * same library): the reference's archs/gaterv2/arch.py; resselt_amd/csrc/gaterv2.hip.  The ctypes mirror and signature rows live in
 * resselt_amd/engine/lib_gaterv2.py, and tests/test_gaterv2_capi.py compares the two field by field.
 *
 * Conventions: split planes [N][planes][H][W][8] of `fmt` (enum rsa_plane_fmt), the lo plane optional; strides in 16-byte units; all
 * arithmetic in f32; no atomics; every reduction runs in a fixed order that depends on (H, W) alone, so a result is bit-identical from
 * run to run.
 */
#ifndef RESSELT_AMD_GATERV2_H
#define RESSELT_AMD_GATERV2_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The token chunk of rsa_gaterv2_linear_attention's partial sums: consecutive tokens (pixels in row-major order). */
#define RSA_GATERV2_TOKEN_CHUNK 128

/* The latent Attention (gaterv2/arch.py:215-250: an l2-normalised linear attention) behind its three 1x1 convolutions, per image over ALL
 * tokens n < N = H W, with m query / key channels and C value channels:
 *   qn[:,n] = q[:,n] * (1 / sqrt(sum_j q[j,n]^2))      kn likewise       the sum an fma chain from 0 over ascending j < m; NO epsilon
 *   ksum[j] = sum_n kn[j,n] + eps        vsum[c] = sum_n v[c,n]        M[j][c] = sum_n kn[j,n] v[c,n]
 *   t[n]    = 1 / (N + sum_j qn[j,n] ksum[j])                            an fma chain from 0 over ascending j
 *   out[c,n] = (vsum[c] + sum_j qn[j,n] M[j][c]) * t[n]                  an fma chain from vsum[c] over ascending j
 * THREE kernels in one call: the partial records [M | ksum | vsum] per chunk of RSA_GATERV2_TOKEN_CHUNK consecutive tokens (fma / add
 * chains from 0 in ascending token order); one ordered finish per image that adds the records in ascending chunk order, adds eps to ksum
 * and leaves M [m][C], ksum [m], vsum [C] at the head of the image's workspace; the apply pass.
 * qkv: ONE plane buffer [q: mp planes | k: mp planes | v: C / 8 planes], mp = ceil(m / 8): the output of one 1x1 convolution whose rows
 * are query_conv, key_conv and value_conv, the q and k rows zero-padded to 8 mp.  Only the first m channels of q and of k are read.
 * out: C / 8 planes; qkv and out must not overlap.
 * A token whose q or k vector is exactly zero gives a non-finite result (1 / 0), as the reference does: it has no epsilon there.
 * Errors: RSA_E_ARG null pointer / bad geometry / bad fmt / reserved field / m > C / workspace too small / overlap;
 * RSA_E_UNSUPPORTED C not a multiple of 8 in 16..1024, m outside 1..64; RSA_E_ALIGN. */
typedef struct rsa_gaterv2_attn_params {
  int32_t batch;               /* 1..65535 */
  int32_t H, W;
  int32_t C;                   /* value channels: multiple of 8, 16..1024 */
  int32_t m;                   /* query / key channels: 1..64, m <= C */
  int32_t fmt;                 /* enum rsa_plane_fmt of qkv and out */
  float eps;                   /* added to ksum (the reference: 1e-6) */
  int32_t reserved0;           /* must be 0 */
  const void* qkv_hi;
  const void* qkv_lo;          /* may be NULL */
  int64_t qkv_plane_stride;    /* 16-byte units */
  int64_t qkv_batch_stride;
  void* out_hi;
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  float* workspace;
  int64_t workspace_bytes;
} rsa_gaterv2_attn_params;
int64_t rsa_gaterv2_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t C, int32_t m); /* <= 0: geometry refused */
int rsa_gaterv2_linear_attention(const rsa_gaterv2_attn_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_GATERV2_H */
